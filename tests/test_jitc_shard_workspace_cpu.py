"""``be_binary_jitmv_workspace_bytes`` covers every sharded scatter call that runs on the workspace it sizes.

``be_binary_jitmv_sharded`` walks a sub-range of the (chunk, lane) classes on a workspace sized for all of them, and the scatter
geometry gives fewer classes more parts (``scatter_geom``, csrc/be_jitc_shared.h): 224 classes run as 224 workgroups, the same
classes cut eight ways as 28 x 9 = 252.  Every workgroup writes ``piece_len`` partial sums, so the size has to hold for the largest
cut, not only for the whole.  The geometry is restated here from the source's constants (read as text); the size is asked of the
library, which needs no device for it."""
import re
from pathlib import Path

import pytest

from brainevent_amd import _lib
from brainevent_amd._dist import post_slice_bounds

SHARED = (Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc' / 'be_jitc_shared.h').read_text()
WG_TARGET = int(re.search(r'#define\s+BE_JIT_WG_TARGET\s+(\d+)', SHARED).group(1))
PIECE_U32, PIECE_U64 = (int(v) for v in re.search(r'kPieceU32\s*=\s*(\d+)\s*,\s*kPieceU64\s*=\s*(\d+)', SHARED).groups())
STRIDE = 32                      # lane stride of the mv matrix


def align(x, a=256):
    return (x + a - 1) // a * a


def partial_bytes(shape1, out_len, n_classes, scalar):
    """Bytes of partial sums a scatter over ``n_classes`` classes writes (``scatter_geom`` + ``k_jit_mv_scatter``, one vector)."""
    chunk = max(1, (shape1 + 3) // 4)
    q_max = (min(chunk, out_len) + STRIDE - 1) // STRIDE
    cap = PIECE_U32 if scalar else PIECE_U64
    pieces = max(1, (q_max + cap - 1) // cap)
    piece_len = max(256, align((q_max + pieces - 1) // pieces))
    parts = max(1, min(WG_TARGET // max(1, n_classes * pieces), 16))
    return n_classes * pieces * parts * piece_len * (4 if scalar else 8)


@pytest.mark.parametrize('shape1,in_len,out_len', [(3000, 3000, 5003), (5003, 3000, 5003), (40000, 3000, 40000), (100, 64, 999),
                                                   (7, 5, 3), (2_000_000, 1000, 2_000_000)])
def test_workspace_holds_every_cut_of_the_classes(shape1, in_len, out_len):
    assert re.search(r'int\s+parts\s*=\s*\(int\)\(BE_JIT_WG_TARGET\s*/', SHARED) and re.search(r'std::min\(parts,\s*16\)', SHARED)
    have = _lib.fn('be_binary_jitmv_workspace_bytes')(shape1, in_len, out_len, 0)
    chunk = max(1, (shape1 + 3) // 4)
    n_classes = (out_len + chunk - 1) // chunk * STRIDE
    head = align(4) + align(in_len * 4)                      # the spike counter and the active list
    for world in range(1, 10):
        for rank in range(world):
            lo, hi = post_slice_bounds(n_classes, world, rank)
            if hi == lo:
                continue
            need = head + align(max(partial_bytes(shape1, out_len, hi - lo, s) for s in (False, True)))
            assert have >= need, (world, rank, hi - lo, have, need)


def test_the_case_that_overran():
    """224 classes, eight ranks: 28 classes x 9 parts = 252 workgroups of 256 fixed-point sums."""
    assert partial_bytes(3000, 5003, 224, False) == 224 * 256 * 8 and partial_bytes(3000, 5003, 28, False) == 252 * 256 * 8
    assert _lib.fn('be_binary_jitmv_workspace_bytes')(3000, 3000, 5003, 0) >= 256 + 12032 + 252 * 256 * 8
