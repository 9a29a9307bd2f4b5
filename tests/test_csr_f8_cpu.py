"""The host side of the FP8 CSR products: the numpy restatement against a brute-force loop over Python ints, the integer decode
table, the quantisation bound, the constants the GPU cases are sized by, and every refusal of the container — raised before any
device call (the device is barred in those tests: asking for it fails the test)."""
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _array as A
from brainevent_amd import _csr_f8 as F
import csr_f8_cases as K

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'brainevent_amd' / 'csrc'
FMTS = sorted(K.E)
FMT_MAX = {'e4m3': 448.0, 'e5m2': 57344.0}


@pytest.fixture
def no_device(monkeypatch):
    def barred(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(A, 'device', barred)
    monkeypatch.setattr(A, 'to_device', barred)
    monkeypatch.setattr(A, 'workspace', barred)


@pytest.mark.parametrize('fmt', FMTS)
def test_q_is_an_integer_within_the_stated_bound_for_every_finite_code(fmt):
    fc = K.finite_codes(fmt)
    assert len(fc) == (254 if fmt == 'e4m3' else 248)
    dec = torch.from_numpy(fc.copy()).view(K.DTYPE[fmt]).to(torch.float64).numpy()
    assert np.isfinite(dec).all()
    q = dec * 2.0 ** K.E[fmt]
    assert np.array_equal(q, np.floor(q)) and np.abs(q).max() == K.Q_MAX[fmt]
    assert np.array_equal(K.q_table(fmt)[fc], q.astype(np.int64))
    # E is the smallest such exponent: the smallest subnormal is 2^-E
    assert np.abs(dec[dec != 0]).min() == 2.0 ** -K.E[fmt]
    # the integer decode the kernels use (be_csr_shared.h, f8_fixed), restated: m for a subnormal, (2^MB + m) << (e - 1) otherwise
    mb = 3 if fmt == 'e4m3' else 2
    for c in fc:
        m_, e_ = int(c) & ((1 << mb) - 1), (int(c) & 0x7f) >> mb
        mag = m_ if e_ == 0 else ((m_ | (1 << mb)) << (e_ - 1))
        assert (-mag if c & 0x80 else mag) == int(K.q_table(fmt)[c]), c
    # R_j cannot overflow below 2^31 entries per column
    assert (1 << 31) * K.Q_MAX[fmt] < (1 << 63)


@pytest.mark.parametrize('fmt', FMTS)
def test_the_restatement_against_a_loop_over_python_ints(fmt):
    m, k = 23, 17
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=5)
    rng = np.random.default_rng(6)
    active = rng.random((3, m)) < 0.5
    dec = torch.from_numpy(np.arange(256, dtype=np.uint8)).view(K.DTYPE[fmt]).to(torch.float64).numpy()
    for scale in (1.0, 0.25, 0.3):
        got = K.expected(codes, indices, indptr, active, k, fmt, scale)
        for b in range(3):
            R = [0] * k
            for i in range(m):
                if active[b, i]:
                    for e in range(indptr[i], indptr[i + 1]):
                        R[indices[e]] += int(dec[codes[e]] * 2 ** K.E[fmt])
            inv = np.ldexp(np.float64(np.float32(scale)), -K.E[fmt])
            want = np.array([np.float32(np.float64(r) * inv) for r in R], dtype=np.float32)
            assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(K.active_of(np.array([1.0, -1.0, np.nan, 0.0, 0.5], dtype=np.float32)), [True, False, False, False, True])
    bits = K.pack_bits(np.arange(70) % 3 == 0)
    assert bits.dtype == np.uint32 and len(bits) == 3 and all(((bits[i // 32] >> (i % 32)) & 1) == (i % 3 == 0) for i in range(70))


def _host_csr(w, indices, indptr, shape):
    """What csr_quantize_fp8 reads of a CSR, on the host."""
    return types.SimpleNamespace(data=torch.from_numpy(w), indices=torch.from_numpy(indices), indptr=torch.from_numpy(indptr),
                                 shape=shape, nse=len(indices), _numpy_result=True)


@pytest.mark.parametrize('fmt', FMTS)
def test_quantisation_follows_the_formula_and_keeps_the_formats_bound(fmt, no_device):
    rng = np.random.default_rng(2)
    m, k = 40, 50
    _, indices, indptr = K.random_matrix(m, k, fmt, seed=3)
    # a wide range of magnitudes: normals, subnormals of the scaled format, zeros
    w = (rng.standard_normal(len(indices)) * np.exp2(rng.integers(-24, 3, len(indices)))).astype(np.float32)
    w[::11] = 0.0
    Q = F.csr_quantize_fp8(_host_csr(w, indices, indptr, (m, k)), fmt)
    scale = float(np.float32(np.abs(w).max()) / np.float32(FMT_MAX[fmt]))
    assert Q.scale == scale and Q.fmt == fmt and Q.shape == (m, k) and Q.nse == len(indices)
    want = (torch.from_numpy(w) / torch.tensor(scale, dtype=torch.float32)).clamp(-FMT_MAX[fmt], FMT_MAX[fmt]).to(K.DTYPE[fmt])
    assert torch.equal(Q.codes.view(torch.uint8), want.view(torch.uint8))
    assert Q.indices.data_ptr() == torch.from_numpy(indices).data_ptr() and Q.indptr.data_ptr() == torch.from_numpy(indptr).data_ptr()
    deq = (Q.codes.to(torch.float32) * torch.tensor(scale, dtype=torch.float32)).numpy().astype(np.float64)
    err, aw = np.abs(deq - w.astype(np.float64)), np.abs(w.astype(np.float64))
    rel, min_normal, sub = ((2.0 ** -4, 2.0 ** -6, 2.0 ** -10) if fmt == 'e4m3' else (2.0 ** -3, 2.0 ** -14, 2.0 ** -17))
    normal = aw >= min_normal * scale
    assert normal.any() and (~normal).any()
    assert (err[normal] <= rel * aw[normal]).all()
    assert (err[~normal] <= sub * scale).all()
    # an all-zero matrix gets scale 1; a scale of the caller's is taken as an f32 number
    Z = F.csr_quantize_fp8(_host_csr(np.zeros_like(w), indices, indptr, (m, k)), fmt)
    assert Z.scale == 1.0 and not bool(Z.codes.view(torch.uint8).any())
    assert F.csr_quantize_fp8(_host_csr(w, indices, indptr, (m, k)), fmt, scale=0.1).scale == float(np.float32(0.1))
    bad = w.copy()
    bad[3] = np.inf
    with pytest.raises(ValueError, match='non-finite'):
        F.csr_quantize_fp8(_host_csr(bad, indices, indptr, (m, k)), fmt)
    with pytest.raises(ValueError, match='positive'):
        F.csr_quantize_fp8(_host_csr(w, indices, indptr, (m, k)), fmt, scale=0.0)
    with pytest.raises(ValueError, match='unknown FP8 format'):
        F.csr_quantize_fp8(_host_csr(w, indices, indptr, (m, k)), 'e3m4')
    with pytest.raises(TypeError, match='h8 plan already stores it|one shared weight'):
        F.csr_quantize_fp8(_host_csr(np.ones(1, np.float32), indices, indptr, (m, k)), fmt)
    with pytest.raises(TypeError, match='float weights'):
        F.csr_quantize_fp8(_host_csr(np.ones(len(indices), np.int32), indices, indptr, (m, k)), fmt)
    assert hasattr(be.CSR, 'quantize_fp8')


def test_the_constants_the_gpu_cases_are_sized_by_are_the_sources():
    plan = (CSRC / 'be_csr_plan.hip').read_text()
    shared = (CSRC / 'be_csr_shared.h').read_text()
    assert re.search(r'constexpr int kD8MaxRow = (\d+);', plan).group(1) == str(K.MAX_ROW)
    assert re.search(r'constexpr int kD8MaxSlices = (\d+);', plan).group(1) == str(K.MAX_SLICES)
    assert re.search(r'constexpr int kD8MaxWidth = (\d+);', plan).group(1) == str(K.MAX_WIDTH)
    assert f'constexpr int kF8ExpE4M3 = {K.E["e4m3"]}, kF8ExpE5M2 = {K.E["e5m2"]};' in shared
    # lanes per block by block_hint: the hints of LPB_VARIANTS select 8, 16 and a wave per block
    eighth = int(re.search(r'constexpr int kD8EighthMaxBlock = (\d+);', plan).group(1))
    quarter = int(re.search(r'constexpr int kD8QuarterMaxBlock = (\d+);', plan).group(1))
    assert 0 < K.LPB_VARIANTS[8] <= eighth < K.LPB_VARIANTS[16] <= quarter < K.LPB_VARIANTS[0]
    assert 'upto(kD8EighthMaxBlock) ? 8 : upto(kD8QuarterMaxBlock) ? 16 : 0' in plan
    # 4 entries per lane-group, 64 lane-groups per wave pass; the q8 kernels are instantiated for both formats at 0 / 8 / 16 lanes
    assert 'const uint32_t ng = H8 ? (tot[s] + 7u) >> 3 : (tot[s] + 3u) >> 2;' in plan and K.LANE_GROUP == 4 and K.WAVE_PASS == 256
    assert 'be_dispatch_int<BE_F8_E4M3, BE_F8_E5M2>(q8_fmt' in plan and 'k_plan_accumulate_q8<decltype(f)::value, decltype(l)::value, FUSED>' in plan
    assert (F.Q8Plan.MAX_ROW, F.Q8Plan.MAX_SLICES, F.Q8Plan.CAP) == (K.MAX_ROW, K.MAX_SLICES, K.MAX_WIDTH)
    assert F.F8_EXP == K.E
    header = (ROOT / 'include' / 'brainevent_amd.h').read_text()
    assert '#define BE_F8_E4M3 0' in header and '#define BE_F8_E5M2 1' in header and K.FMT_CODE == {'e4m3': 0, 'e5m2': 1}


def test_fp8_stays_out_of_the_weight_dtypes_and_the_plan_layouts():
    assert set(A._W_CODE) == {torch.float32, torch.float64, torch.float16, torch.bfloat16}
    assert A._W_CODE == {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
    with pytest.raises(AssertionError, match='floating-point'):
        A.wcode(torch.zeros(4).to(torch.float8_e5m2))
    with pytest.raises(ValueError, match="'u16', 'd8', 'h8' or None"):
        be.ScatterPlan._choose_geometry(4, 4, 4, False, 1, None, None, 'q8')
    header = (ROOT / 'include' / 'brainevent_amd.h').read_text()
    assert re.findall(r'#define BE_PLAN_\w+ \d', header) == ['#define BE_PLAN_U16 0', '#define BE_PLAN_D8 1', '#define BE_PLAN_H8 2']


@pytest.mark.parametrize('fmt', FMTS)
def test_the_container_on_the_host(fmt, no_device):
    fc = K.finite_codes(fmt)
    rows = [([3, 0, 3], fc[[1, 2, 3]]), ([], []), ([5], fc[[200]])]
    codes, indices, indptr = K.from_rows(rows, 6)
    W = be.Float8CSR((codes, indices, indptr), shape=(3, 6), scale=0.5, fmt=fmt)
    assert W.fmt == fmt and W.dtype == K.DTYPE[fmt] and W.shape == (3, 6) and W.nse == 4 and W.scale == 0.5 and W.ndim == 2
    assert 'Float8CSR' in repr(W) and fmt in repr(W)
    dec = torch.from_numpy(codes.copy()).view(K.DTYPE[fmt]).float().numpy() * np.float32(0.5)
    dense = np.zeros((3, 6), np.float32)
    np.add.at(dense, ([0, 0, 0, 2], indices), dec)
    assert isinstance(W.todense(), np.ndarray) and np.array_equal(W.todense(), dense)
    Wt = be.Float8CSR((torch.from_numpy(codes.copy()).view(K.DTYPE[fmt]), torch.from_numpy(indices), torch.from_numpy(indptr).long()),
                      shape=(3, 6))
    assert Wt.scale == 1.0 and Wt.fmt == fmt and isinstance(Wt.todense(), torch.Tensor) and Wt.indptr.dtype in (torch.int32, torch.int64)
    assert be.Float8CSR((codes, indices, indptr), shape=(3, 6), scale=0.1, fmt=fmt).scale == float(np.float32(0.1))


def test_container_refusals(no_device):
    codes, indices, indptr = K.from_rows([([1, 2], [8, 9]), ([0], [16])], 6)
    mk = lambda **kw: be.Float8CSR((codes, indices, indptr), **{'shape': (2, 6), 'fmt': 'e4m3', **kw})
    W = mk()
    x = np.ones(6, dtype=np.float32)
    with pytest.raises(TypeError, match=r'event operands only.*tocsr\(\)'):
        W @ x
    with pytest.raises(TypeError, match=r'event operands only.*tocsr\(\)'):
        W.__rmatmul__(np.ones(2, dtype=np.float32))
    with pytest.raises(TypeError, match=r'event operands only.*tocsr\(\)'):
        torch.ones(3, 2) @ W
    with pytest.raises(NotImplementedError, match=r'gather direction, W8 @ events'):
        W @ be.BinaryArray(np.ones(6, dtype=bool))
    for op in (lambda: W + 1, lambda: 1 + W, lambda: W - W, lambda: W * 2.0, lambda: 2.0 * W, lambda: W / 2, lambda: -W, lambda: abs(W),
               lambda: W ** 2, lambda: W[0], lambda: W.slice_rows([0]), lambda: W.solve(x), lambda: W.update_on_pre(x, x),
               lambda: W.update_on_post(x, x), lambda: W.update_on_binary_pre(x, x), lambda: W.update_on_binary_post(x, x),
               lambda: W.diag_add(x), lambda: W.with_data(x)):
        with pytest.raises(TypeError, match='read-only'):
            op()
    # shapes and gradients are checked before the device is asked for
    with pytest.raises(ValueError, match='not aligned'):
        be.BinaryArray(np.ones(5, dtype=bool)) @ W
    with pytest.raises(ValueError, match='not aligned'):
        be.BinaryArray(np.ones((3, 5), dtype=bool)) @ W
    with pytest.raises(TypeError, match='no gradients'):
        be.BinaryArray(torch.ones(2, requires_grad=True)) @ W
    # construction
    with pytest.raises(ValueError, match="fmt='e4m3' or fmt='e5m2'"):
        mk(fmt=None)
    with pytest.raises(ValueError, match='unknown FP8 format'):
        mk(fmt='e3m4')
    with pytest.raises(ValueError, match='does not match'):
        be.Float8CSR((torch.zeros(3).to(torch.float8_e5m2), indices, indptr), shape=(2, 6), fmt='e4m3')
    with pytest.raises(TypeError, match='uint8 codes'):
        be.Float8CSR((np.zeros(3, dtype=np.float32), indices, indptr), shape=(2, 6), fmt='e4m3')
    with pytest.raises(ValueError, match='one-dimensional'):
        be.Float8CSR((np.zeros((3, 1), dtype=np.uint8), indices, indptr), shape=(2, 6), fmt='e4m3')
    with pytest.raises(ValueError, match='3 indices'):
        be.Float8CSR((np.zeros(2, dtype=np.uint8), indices, indptr), shape=(2, 6), fmt='e4m3')
    with pytest.raises(ValueError, match='finite'):
        mk(scale=float('nan'))
    with pytest.raises(TypeError, match='requires grad'):
        mk(scale=torch.ones((), requires_grad=True))
    with pytest.raises(ValueError, match='out of bounds'):
        mk(shape=(2, 2))
    with pytest.raises(ValueError, match='indptr length'):
        mk(shape=(3, 6))
    with pytest.raises(TypeError, match='integer'):
        be.Float8CSR((codes, indices.astype(np.float32), indptr), shape=(2, 6), fmt='e4m3')
    for fmt, mask in K.NONFINITE_MASK.items():
        for c in (c for c in range(256) if (c & mask) == mask):
            bad = codes.copy()
            bad[1] = c
            with pytest.raises(ValueError, match='non-finite'):
                be.Float8CSR((bad, indices, indptr), shape=(2, 6), fmt=fmt)
