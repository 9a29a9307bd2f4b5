"""The host side of the FP8 dense products: quantize_fp8 against its stated formula, the Float8Dense container, and every refusal —
raised before any device call (no GPU here: a device call would raise KernelNotAvailableError instead)."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _array as A
from brainevent_amd import _dense_f8 as F
from dense_f8_cases import FORMATS, NONFINITE_MASK, finite_codes

FMTS = sorted(FORMATS)
FMT_MAX = {'e4m3': 448.0, 'e5m2': 57344.0}


def formula(W, fmt, scale):
    return (W.float() / torch.tensor(scale, dtype=torch.float32)).clamp(-FMT_MAX[fmt], FMT_MAX[fmt]).to(FORMATS[fmt])


@pytest.mark.parametrize('fmt', FMTS)
def test_quantize_fp8_is_the_stated_formula(fmt):
    W = torch.from_numpy(np.random.default_rng(1).standard_normal((37, 29)).astype(np.float32)) * 3
    Q = be.quantize_fp8(W, fmt=fmt)
    scale = float(np.float32(float(W.abs().max())) / np.float32(FMT_MAX[fmt]))
    assert Q.scale == scale and Q.fmt == fmt and Q.dtype == FORMATS[fmt] and Q.shape == (37, 29)
    assert torch.equal(Q.codes.view(torch.uint8), formula(W, fmt, scale).view(torch.uint8))
    assert float(Q.codes.float().abs().max()) == FMT_MAX[fmt]                      # amax lands on the format's largest number
    assert torch.equal(Q.todense(), Q.codes.float() * torch.tensor(scale, dtype=torch.float32))
    assert Q.todense(torch.float64).dtype == torch.float64
    # a scale of the caller's; numpy in -> numpy out
    Qn = be.quantize_fp8(W.numpy(), fmt=fmt, scale=0.25)
    assert Qn.scale == 0.25 and isinstance(Qn.todense(), np.ndarray)
    assert torch.equal(Qn.codes.view(torch.uint8), formula(W, fmt, 0.25).view(torch.uint8))
    assert be.Dense is not None and 'Float8Dense' in repr(Q) and fmt in repr(Q)


@pytest.mark.parametrize('fmt', FMTS)
def test_quantize_fp8_clamps_and_takes_an_all_zero_matrix(fmt):
    """Values past +-FMT_MAX * scale are clamped: without the clamp torch's cast gives NaN (e4m3fn) / inf (e5m2)."""
    big = FMT_MAX[fmt] * 4
    W = torch.tensor([[big, -big, 1.0, 0.0], [FMT_MAX[fmt], -FMT_MAX[fmt], 0.5, -0.0]])
    unclamped = W.to(FORMATS[fmt]).float()
    assert not bool(torch.isfinite(unclamped).all())                                # what the clamp is for
    Q = be.quantize_fp8(W, fmt=fmt, scale=1.0)
    d = Q.codes.float()
    assert bool(torch.isfinite(d).all())
    assert d[0, 0] == FMT_MAX[fmt] and d[0, 1] == -FMT_MAX[fmt] and d[1, 0] == FMT_MAX[fmt] and d[0, 2] == 1.0 and d[1, 2] == 0.5
    Z = be.quantize_fp8(torch.zeros(3, 5), fmt=fmt)
    assert Z.scale == 1.0 and not bool(Z.codes.view(torch.uint8).any()) and not bool(Z.todense().any())
    with pytest.raises(ValueError, match='non-finite'):
        be.quantize_fp8(torch.tensor([[1.0, float('inf')]]), fmt=fmt)
    with pytest.raises(ValueError, match='positive'):
        be.quantize_fp8(torch.ones(2, 2), fmt=fmt, scale=0.0)
    with pytest.raises(ValueError, match='unknown FP8 format'):
        be.quantize_fp8(torch.ones(2, 2), fmt='e3m4')
    with pytest.raises(TypeError):
        be.quantize_fp8(torch.ones(2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match='two-dimensional'):
        be.quantize_fp8(torch.ones(4))


@pytest.mark.parametrize('fmt', FMTS)
def test_uint8_codes_round_trip(fmt):
    c = finite_codes(fmt).reshape(16, 16)
    Q = be.Float8Dense(c, scale=0.5, fmt=fmt)
    assert Q.fmt == fmt and Q.dtype == FORMATS[fmt] and Q.shape == (16, 16) and Q.scale == 0.5 and Q.ndim == 2
    assert np.array_equal(Q.codes.view(torch.uint8).numpy(), c)
    dec = torch.from_numpy(c.copy()).view(FORMATS[fmt]).float().numpy()
    assert isinstance(Q.todense(), np.ndarray) and np.array_equal(Q.todense(), dec * np.float32(0.5))
    Qt = be.Float8Dense(torch.from_numpy(c.copy()), fmt=fmt)                           # a uint8 tensor
    assert Qt.scale == 1.0 and torch.equal(Qt.todense(), torch.from_numpy(dec))
    Qf = be.Float8Dense(torch.from_numpy(c.copy()).view(FORMATS[fmt]))                 # the FP8 tensor itself
    assert Qf.fmt == fmt and torch.equal(Qf.todense(), torch.from_numpy(dec))
    T = Q.T
    assert T.shape == (16, 16) and T.scale == 0.5 and np.array_equal(T.codes.view(torch.uint8).numpy(), c.T)
    assert np.array_equal(Q.transpose().todense(), Q.todense().T)
    assert be.Float8Dense(c, scale=0.1, fmt=fmt).scale == float(np.float32(0.1))       # the scale is an f32 number


@pytest.mark.parametrize('fmt', FMTS)
def test_non_finite_codes_are_refused_before_any_device_call(fmt):
    m = NONFINITE_MASK[fmt]
    bad_codes = [c for c in range(256) if (c & m) == m]
    assert len(bad_codes) == (2 if fmt == 'e4m3' else 8)
    decoded = torch.tensor(bad_codes, dtype=torch.uint8).view(FORMATS[fmt]).float()
    assert not bool(torch.isfinite(decoded).any())                                     # the byte test names exactly inf / NaN
    assert bool(torch.isfinite(torch.from_numpy(finite_codes(fmt)).view(FORMATS[fmt]).float()).all())
    s1, s2 = np.ones(4, dtype=bool), np.ones((4, 3), dtype=bool)
    for c in bad_codes:
        u = np.zeros((4, 4), dtype=np.uint8)
        u[2, 1] = c
        with pytest.raises(ValueError, match='non-finite'):
            be.Float8Dense(u, fmt=fmt)
        w = torch.from_numpy(u).view(FORMATS[fmt])
        with pytest.raises(ValueError, match='non-finite'):
            be.Float8Dense(w)
        for call in (lambda: be.binary_densemv(w, s1, transpose=True), lambda: be.binary_densemv(w, s1, transpose=False),
                     lambda: be.binary_densemm(w, s2, transpose=True), lambda: be.binary_densemm(w, s2, transpose=False),
                     lambda: be.BinaryArray(s1) @ w, lambda: w @ be.BinaryArray(s1), lambda: be.BinaryArray(s2.T) @ w):
            with pytest.raises(ValueError, match='non-finite'):
                call()


def test_the_finite_check_runs_once_per_tensor_version(monkeypatch):
    w = torch.zeros((4, 4), dtype=torch.uint8).view(torch.float8_e5m2)
    F.check_finite(w)
    ref, version = F._checked[id(w)]
    assert ref() is w and version == w._version
    with monkeypatch.context() as mp:
        mp.setattr(F, '_NONFINITE_MASK', {})           # a second read would fail here: an unchanged tensor is not read again
        F.check_finite(w)
        with pytest.raises(KeyError):
            F.check_finite(torch.zeros((2, 2), dtype=torch.uint8).view(torch.float8_e5m2))
    w.view(torch.uint8)[0, 0] = 0x7c                  # +inf, written in place: a new version, read again
    assert w._version != version
    with pytest.raises(ValueError, match='non-finite'):
        F.check_finite(w)
    key = id(w)
    del w, ref
    assert key not in F._checked                        # the cache does not keep tensors alive


def test_container_refusals():
    Q = be.Float8Dense(np.zeros((4, 6), dtype=np.uint8), fmt='e4m3')
    x = np.ones(6, dtype=np.float32)
    with pytest.raises(TypeError, match='event operands only'):
        Q @ x
    with pytest.raises(TypeError, match='event operands only'):
        Q @ torch.ones(6, 2)
    with pytest.raises(TypeError, match='event operands only'):
        Q.__rmatmul__(np.ones(4, dtype=np.float32))
    for op in (lambda: Q + 1, lambda: 1 + Q, lambda: Q - Q, lambda: Q * 2.0, lambda: 2.0 * Q, lambda: Q / 2, lambda: -Q, lambda: abs(Q),
               lambda: Q ** 2, lambda: Q[0], lambda: Q[:, 1], lambda: Q.solve(x), lambda: Q.update_on_pre(x, x),
               lambda: Q.update_on_post(x, x), lambda: Q.update_on_binary_pre(x, x), lambda: Q.diag_add(x), lambda: Q.with_data(x)):
        with pytest.raises(TypeError, match='read-only'):
            op()
    # shapes are checked before the device is asked for
    with pytest.raises(ValueError, match='not aligned'):
        Q @ be.BinaryArray(np.ones(5, dtype=bool))
    with pytest.raises(ValueError, match='not aligned'):
        be.BinaryArray(np.ones((3, 5), dtype=bool)) @ Q
    # construction
    with pytest.raises(ValueError, match="fmt='e4m3' or fmt='e5m2'"):
        be.Float8Dense(np.zeros((2, 2), dtype=np.uint8))
    with pytest.raises(ValueError, match='unknown FP8 format'):
        be.Float8Dense(np.zeros((2, 2), dtype=np.uint8), fmt='e3m4')
    with pytest.raises(ValueError, match='does not match'):
        be.Float8Dense(torch.zeros(2, 2).to(torch.float8_e5m2), fmt='e4m3')
    with pytest.raises(TypeError, match='uint8 codes'):
        be.Float8Dense(np.zeros((2, 2), dtype=np.float32), fmt='e4m3')
    with pytest.raises(ValueError, match='two-dimensional'):
        be.Float8Dense(np.zeros(4, dtype=np.uint8), fmt='e4m3')
    with pytest.raises(ValueError, match='finite'):
        be.Float8Dense(np.zeros((2, 2), dtype=np.uint8), scale=float('inf'), fmt='e4m3')
    with pytest.raises(TypeError, match='requires grad'):
        be.Float8Dense(np.zeros((2, 2), dtype=np.uint8), scale=torch.ones((), requires_grad=True), fmt='e4m3')


def test_gradients_are_refused():
    w = torch.zeros(4, 6).to(torch.float8_e4m3fn)
    s = torch.ones(4, requires_grad=True)
    with pytest.raises(TypeError, match='no gradients'):
        be.binary_densemv(w, s, transpose=True)
    with pytest.raises(TypeError, match='no gradients'):
        be.binary_densemm(w, torch.ones(4, 2, requires_grad=True), transpose=True)
    with pytest.raises(TypeError, match='no gradients'):
        be.Float8Dense(w).__rmatmul__(be.BinaryArray(s))


def test_the_other_families_keep_refusing_fp8():
    w = torch.zeros(4).to(torch.float8_e4m3fn)
    with pytest.raises(AssertionError, match='floating-point'):
        A.wcode(w)
    assert set(A._W_CODE) == {torch.float32, torch.float64, torch.float16, torch.bfloat16}
