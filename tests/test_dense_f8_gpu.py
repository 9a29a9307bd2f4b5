"""The FP8 dense products (csrc/be_dense_f8.hip) on the device, compared exactly (no tolerance) with the reference of
tests/dense_f8_cases.py, at the smallest shapes at which each loop can go wrong.  tests/test_dense_f8_thresholds_cpu.py holds the
CONSTS table the shapes are sized by against the kernels' source."""
import numpy as np
import pytest
import torch

import dense_f8_cases as C
from dense_f8_cases import FORMATS, K

pytestmark = pytest.mark.gpu
FMTS = sorted(FORMATS)


def dev(codes):
    return codes.cuda().contiguous()


# ================================================================================================= decode table
@pytest.mark.parametrize('fmt', FMTS)
def test_decode_table_mfma(be, fmt):
    """Every finite code through k8_densemm_mfma: a one-hot batch of 256 rows (eight passes) picks one table row each, so every k
    position of the MFMA operand carries every code once."""
    table, dec = C.decode_table(fmt)
    Wd = torch.from_numpy(table).cuda().view(FORMATS[fmt])
    S = np.eye(256, dtype=bool)
    assert C.route((256, 32), 256, True) == 't_mfma' and C.passes(256) == 8
    ref = np.repeat(dec[:, None], 32, axis=1)
    assert np.array_equal(C.reference(Wd, S, True), ref)
    C.run(Wd, S, 'bool', True, ref, 'decode table mfma')


@pytest.mark.parametrize('fmt', FMTS)
def test_decode_table_vector_routes(be, fmt):
    """The same table through the packed converts of the vector S @ W8 kernel (1-D spikes, and batches of 4) and through the
    one-code convert of its scalar-load variant (a misaligned view)."""
    from brainevent_amd import _dense_f8 as F
    table, dec = C.decode_table(fmt)
    Wd = torch.from_numpy(table).cuda().view(FORMATS[fmt])
    Wm = C.misaligned(Wd)
    assert C.route((256, 32), 1, True) == C.route((256, 32), 4, True) == 't_vec16' and C.route((256, 32), 4, True, False) == 't_vec1'
    eye = torch.eye(256, dtype=torch.bool, device='cuda')
    got1 = torch.stack([be.binary_densemv(Wd, eye[c], transpose=True) for c in range(256)])
    got4 = torch.cat([F.dense_f8_batched(Wd, 1.0, eye[c:c + 4], 0, True) for c in range(0, 256, 4)])
    got4m = torch.cat([F.dense_f8_batched(Wm, 1.0, eye[c:c + 4], 0, True) for c in range(0, 256, 4)])
    ref = np.repeat(dec[:, None], 32, axis=1)
    for name, got in (('1-D', got1), ('nb=4', got4), ('nb=4 scalar loads', got4m)):
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), ref), (fmt, name)


@pytest.mark.parametrize('fmt', FMTS)
def test_decode_table_no_transpose(be, fmt):
    """W8 @ S.T on the transposed table [32, 256]: out[b, i] = decode(b); 16-B loads and the scalar-load variant."""
    table, dec = C.decode_table(fmt)
    Wd = torch.from_numpy(np.ascontiguousarray(table.T)).cuda().view(FORMATS[fmt])
    S = np.eye(256, dtype=bool)
    ref = np.repeat(dec[:, None], 32, axis=1)
    C.run(Wd, S, 'bool', False, ref, 'decode table nt', expect='nt_vec16')
    C.run(C.misaligned(Wd), S, 'bool', False, ref, 'decode table nt scalar', expect='nt_vec1')


# ================================================================================================= MFMA route
@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('name,seed', [('two_chunks_16_parts', 11), ('seven_parts', 12), ('one_part', 13), ('empty_ranges', 14)])
def test_mfma_parts_and_chunks(be, name, seed, fmt):
    C.cross_mfma()
    (k, n), nb, firing = C.MFMA_CASES[name]
    S = C.draw(seed, nb, k, firing, last=True)
    codes = C.codes_of(C.int_weights(seed, (k, n)), fmt)
    C.run(dev(codes), S, 'bool', True, C.reference(codes, S, True), name, expect='t_mfma')


@pytest.mark.parametrize('nb', C.MFMA_NBS)
def test_mfma_batch_sizes_silent_rows_and_silent_pass(be, nb):
    """nb in {8, 9, 32, 33, 65} on the shape with empty K ranges and a partly filled column tile; batch row 1 is silent, and from
    33 rows on every row of the later passes is: a pass without any spike."""
    (k, n), _, firing = C.MFMA_CASES['empty_ranges']
    S = C.draw(30 + nb, nb, k, firing, last=True)
    S[1] = False
    S[K['k8MaxChunk']:] = False
    assert C.passes(nb) == (1 if nb <= 32 else 2 if nb <= 64 else 3) and (nb <= 32 or C.union(S, 32) == 0)
    for fmt in FMTS:
        codes = C.codes_of(C.int_weights(nb, (k, n)), fmt)
        got = C.run(dev(codes), S, 'bool', True, C.reference(codes, S, True), f'nb={nb}', expect='t_mfma')
        assert not bool(got[1].any())


def test_mfma_no_spikes_at_all(be):
    (k, n), nb, _ = C.MFMA_CASES['empty_ranges']
    S = np.zeros((nb, k), dtype=bool)
    codes = C.codes_of(C.int_weights(3, (k, n)), 'e4m3')
    C.run(dev(codes), S, 'bool', True, np.zeros((nb, n), np.float32), 'no spikes', expect='t_mfma')


# ================================================================================================= list building
@pytest.mark.parametrize('name', sorted(C.SCAN_CASES))
def test_list_building_past_the_self_scan_limit(be, name):
    """More than 1024 tiles of rows: the scan launch (its second trip) behind the fused masks + counts, and the general four
    launches of two batch groups; and exactly 1024 tiles, the last shape without a scan launch."""
    C.cross_scan()
    (k, n), nb, firing, how, expect = C.SCAN_CASES[name]
    S = C.draw(100, nb, k, firing, last=True)
    codes = C.codes_of(C.int_weights(101, (k, n)), 'e4m3')
    C.run(dev(codes), S, 'bool', True, C.reference(codes, S, True), f'{name} ({how})', expect=expect)


def test_spike_operand_off_alignment(be):
    """Byte spikes with k % 8 == 0 take 8-byte loads in the fused mask kernel; an operand one byte off must not."""
    k, n, nb = 4096 + 64, 48, 3
    S = C.draw(110, nb, k, 0.3, last=True)
    codes = C.codes_of(C.int_weights(111, (k, n)), 'e5m2')
    ref = C.reference(codes, S, True)
    from brainevent_amd import _array as A, _dense_f8 as F
    buf = torch.zeros(S.size + 16, dtype=torch.bool, device='cuda')
    view = buf[1:1 + S.size].view(S.shape)
    view.copy_(torch.from_numpy(S))
    assert k % 8 == 0 and view.data_ptr() % 8 == 1 and view.is_contiguous() and C.list_launches(k, nb, True, n=n) == 'fused+self_scan'
    for op in (view, torch.from_numpy(S).cuda()):
        got = F.dense_f8_batched(dev(codes), 1.0, op, A.BE_SPIKE_BOOL, True)
        assert np.array_equal(got.cpu().numpy(), ref), op.data_ptr() % 8


# ================================================================================================= vector routes
@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('name', sorted(C.T_VEC_CASES))
def test_vector_route_s_at_w(be, name, fmt):
    C.cross_t_vec()
    (k, n), nb, firing, aligned, expect = C.T_VEC_CASES[name]
    seed = {'more_rows_than_parts': 21, 'fewer_rows_than_parts': 22}.get(name, 23)
    S = C.draw(seed, nb, k, firing, last=True)
    codes = C.codes_of(C.int_weights(seed, (k, n)), fmt)
    Wd = dev(codes) if aligned else C.misaligned(dev(codes))
    C.run(Wd, S, 'bool', True, C.reference(codes, S, True), name, expect=expect)


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('name', sorted(C.NT_CASES))
def test_vector_route_w_at_s(be, name, fmt):
    C.cross_nt()
    (m, k), nb, firing, aligned, expect = C.NT_CASES[name]
    S = C.draw(40, nb, k, firing, last=True)
    codes = C.codes_of(C.int_weights(41, (m, k)), fmt)
    Wd = dev(codes) if aligned else C.misaligned(dev(codes))
    C.run(Wd, S, 'bool', False, C.reference(codes, S, False), name, expect=expect)


# ================================================================================================= spike kinds, scale
@pytest.mark.parametrize('kind', ['bool', 'float', 'bits'])
@pytest.mark.parametrize('case', range(len(C.KIND_CASES)))
def test_spike_kinds_on_every_route(be, case, kind):
    C.cross_kinds()
    shape, nb, transpose, aligned, expect = C.KIND_CASES[case]
    kk = shape[0] if transpose else shape[1]
    S = C.draw(50 + case, nb, kk, 0.4, last=True)
    for fmt in FMTS:
        codes = C.codes_of(C.int_weights(51 + case, shape), fmt)
        C.run(dev(codes), S, kind, transpose, C.reference(codes, S, transpose), f'kinds {expect}', expect=expect)


@pytest.mark.parametrize('scale', [1.0, 2.0 ** -3, 0.1])
@pytest.mark.parametrize('case', [0, 1, 3])
def test_scale_is_one_rounded_multiply(be, case, scale):
    """scale 1 and 2^-3 are equalities with the plain sum; 0.1 equals np.float32(sum) * np.float32(0.1)."""
    shape, nb, transpose, aligned, expect = C.KIND_CASES[case]
    kk = shape[0] if transpose else shape[1]
    S = C.draw(60, nb, kk, 0.4, last=True)
    codes = C.codes_of(C.int_weights(61, shape), 'e5m2')
    plain = C.reference(codes, S, transpose)
    ref = C.reference(codes, S, transpose, scale)
    assert np.array_equal(ref, plain * np.float32(scale)) and (scale == 0.1 or np.array_equal(ref.astype(np.float64), plain * scale))
    C.run(dev(codes), S, 'bool', transpose, ref, f'scale {expect}', scale=scale, expect=expect)


# ================================================================================================= empty shapes
@pytest.mark.parametrize('transpose', [True, False])
def test_empty_shapes(be, transpose):
    from brainevent_amd import _array as A
    from brainevent_amd._lib import call, fn
    # k = 0: zeros, written by the fill kernel into a poisoned output
    nb, out_len = 5, 37
    shape = (0, out_len) if transpose else (out_len, 0)
    W = torch.zeros(shape, dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    out = torch.full((nb, out_len), float('nan'), device='cuda')
    sp = torch.zeros((nb, 0), dtype=torch.bool, device='cuda')
    ws = A.workspace(fn('be_binary_densemm_f8_workspace_bytes')(shape[0], shape[1], nb, int(transpose), 0))
    call('be_binary_densemm_f8', A.ptr(W), 0, 1.0, A.ptr(sp), A.BE_SPIKE_BOOL, A.ptr(out), shape[0], shape[1], nb, int(transpose),
         A.ptr(ws), ws.numel(), A.stream_ptr())
    assert bool((out == 0).all())
    # nb = 0 and an empty output: nothing to do, BE_OK
    codes = dev(C.codes_of(C.int_weights(1, (20, 32)), 'e4m3'))
    kk = 20 if transpose else 32
    r = be.binary_densemm(codes, torch.zeros((kk, 0), dtype=torch.bool, device='cuda'), transpose=transpose)
    assert tuple(r.shape) == ((32 if transpose else 20), 0) and r.dtype == torch.float32
    shape = (20, 0) if transpose else (0, 20)
    W0 = torch.zeros(shape, dtype=torch.uint8, device='cuda').view(torch.float8_e5m2)
    r = be.binary_densemm(W0, torch.ones((20, 3), dtype=torch.bool, device='cuda'), transpose=transpose)
    assert tuple(r.shape) == (0, 3) and r.dtype == torch.float32


def test_c_abi_refusals(be):
    """An unknown format, an unknown spike dtype and a small workspace return the error codes of be_binary_densemm."""
    from brainevent_amd import _array as A
    from brainevent_amd._lib import fn
    f = fn('be_binary_densemm_f8')
    W = dev(C.codes_of(C.int_weights(1, (20, 32)), 'e4m3'))
    sp = torch.ones((2, 20), dtype=torch.bool, device='cuda')
    out = torch.zeros((2, 32), device='cuda')
    ws = A.workspace(fn('be_binary_densemm_f8_workspace_bytes')(20, 32, 2, 1, 0))

    def status(fmt=0, sd=A.BE_SPIKE_BOOL, ws_bytes=None):
        return f(A.ptr(W), fmt, 1.0, A.ptr(sp), sd, A.ptr(out), 20, 32, 2, 1, A.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                 A.stream_ptr())
    assert status() == 0
    assert status(fmt=2) == -1 and 'FP8 format' in be._lib.last_error()
    assert status(sd=A.BE_SPIKE_IDS) == -1
    assert status(ws_bytes=16) == -2


# ================================================================================================= Python surface
@pytest.mark.parametrize('fmt', FMTS)
def test_container_equals_functional_calls(be, fmt):
    k, n, nb = 80, 48, 9
    codes = C.codes_of(C.int_weights(70, (k, n)), fmt)
    Wd = dev(codes)
    Q = be.Float8Dense(Wd)
    S = C.draw(71, nb, k, 0.4, last=True)
    St = C.draw(72, nb, n, 0.4, last=True)
    Sd, Std = torch.from_numpy(S).cuda(), torch.from_numpy(St).cuda()
    # events @ W8 (transpose=True), 2-D and 1-D, every event container
    ref = C.reference(codes, S, True)
    for ev in (be.BinaryArray(Sd), be.BitPackedBinary(Sd), be.CompactBinary.from_array(Sd)):
        assert np.array_equal((ev @ Q).cpu().numpy(), ref), type(ev).__name__
    assert np.array_equal((be.BinaryArray(Sd) @ Wd).cpu().numpy(), ref)
    assert np.array_equal(be.binary_densemm(Wd, Sd.T, transpose=True).T.cpu().numpy(), ref)
    for ev in (be.BinaryArray(Sd[0]), be.BitPackedBinary(Sd[0]), be.CompactBinary.from_array(Sd[0])):
        assert np.array_equal((ev @ Q).cpu().numpy(), ref[0]), type(ev).__name__
    assert np.array_equal(be.binary_densemv(Wd, Sd[0], transpose=True).cpu().numpy(), ref[0])
    # W8 @ events (transpose=False): events are [n, nb]
    reft = C.reference(codes, St, False)
    for ev in (be.BinaryArray(Std.T), be.BitPackedBinary(Std.T.contiguous())):
        assert np.array_equal((Q @ ev).cpu().numpy(), reft.T), type(ev).__name__
    assert np.array_equal((Wd @ be.BinaryArray(Std.T)).cpu().numpy(), reft.T)
    assert np.array_equal(be.binary_densemm(Wd, Std.T, transpose=False).cpu().numpy(), reft.T)
    assert np.array_equal((Q @ be.BinaryArray(Std[0])).cpu().numpy(), reft[0])
    assert np.array_equal((Q @ be.BitPackedBinary(Std[0])).cpu().numpy(), reft[0])
    assert np.array_equal(be.binary_densemv(Wd, Std[0], transpose=False).cpu().numpy(), reft[0])
    # the transposed container, and numpy in -> numpy out
    assert np.array_equal((Q.T @ be.BinaryArray(Sd.T)).cpu().numpy(), ref.T)
    Qn = be.Float8Dense(codes.view(torch.uint8).numpy(), fmt=fmt)
    r = be.BinaryArray(S) @ Qn
    assert isinstance(r, np.ndarray) and r.dtype == np.float32 and np.array_equal(r, ref)


@pytest.mark.parametrize('fmt', FMTS)
def test_quantize_then_product(be, fmt):
    """quantize_fp8(W) followed by a product equals the reference computed from the same codes and scale."""
    k, n, nb = 80, 48, 9
    W = torch.from_numpy(C.int_weights(80, (k, n)).astype(np.float32) * 0.5)
    Q = be.quantize_fp8(W.cuda(), fmt=fmt)
    assert Q.scale == float(np.float32(4.0) / np.float32(be._dense_f8.FMT_MAX[fmt]))
    S = C.draw(81, nb, k, 0.4, last=True)
    ref = C.reference(Q.codes, S, True, Q.scale)          # (asserts that the decoded codes' sums are exact)
    got = be.BinaryArray(torch.from_numpy(S).cuda()) @ Q
    assert np.array_equal(got.cpu().numpy(), ref)
    D = be.Dense(W.cuda()).quantize(fmt)
    assert D.scale == Q.scale and torch.equal(D.codes.view(torch.uint8), Q.codes.view(torch.uint8))


def test_graph_capture_replays_with_new_spikes(be):
    k, n, nb = 300, 272, 9
    codes = C.codes_of(C.int_weights(90, (k, n)), 'e4m3')
    Q = be.Float8Dense(dev(codes), scale=0.5)
    Wd = dev(codes)
    S0, S1 = C.draw(91, nb, k, 0.3), C.draw(92, nb, k, 0.3)
    static = torch.from_numpy(S0).cuda()
    step = be.capture_step(lambda: (be.BinaryArray(static) @ Q, be.BinaryArray(static) @ Wd, be.BinaryArray(static[0]) @ Q))
    static.copy_(torch.from_numpy(S1))
    a, b, c = step()
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), C.reference(codes, S1, True, 0.5))
    assert np.array_equal(b.cpu().numpy(), C.reference(codes, S1, True))
    assert np.array_equal(c.cpu().numpy(), C.reference(codes, S1[:1], True, 0.5)[0])
    assert torch.equal(a, be.BinaryArray(static) @ Q)
