"""Plastic mode (``prepare(plastic=(w_min, w_max))``), host side: the bound-certified exponent against hand-computed cases, the
argument checks that need no device, and the C header's declarations of the new entry points (no GPU needed)."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _plasticity as P

HEADER = Path(__file__).resolve().parent.parent / 'include' / 'brainevent_amd.h'


# ------------------------------------------------------------------------------------------------------------ the exponent
@pytest.mark.parametrize('cmax, bound, want', [
    (40, 2.0 ** 20, 36),      # 40 * 2^20 = 2^25.32: ceil = 26
    (3, 1.0, 60),             # 3 = 2^1.58: ceil = 2
    (1000, 0.75, 52),         # 750 = 2^9.55: ceil = 10
    (7, 2.0 ** -30, 89),      # 7 * 2^-30 = 2^-27.19: ceil = -27
    (4, 0.25, 61),            # exactly 2^0: the sum of 4 weights at the bound could reach 2^62 itself at e = 62 -> one below
    (1 << 20, 2.0 ** 11, 30),  # exactly 2^31 -> 61 - 31
    (5, 0.0, 150),            # nothing can overflow: the largest exponent there is
    (0, 1.0, 150),            # no entries
    (1, 2.0 ** 100, -39),     # 2^100 exactly -> 61 - 100
    (1, 2.0 ** 127, -66),
    (1 << 30, 2.0 ** 127, -90),   # clamped from below
    (1, 2.0 ** -140, 150),    # clamped from above
])
def test_exponent_bound_hand_cases(cmax, bound, want):
    e = P.plastic_exponent_bound(cmax, bound)
    assert e == want
    assert P.plastic_exponent_bound(cmax, -bound) == want            # |bound|
    if 0 < bound and cmax > 0 and P.EXP_MIN < e < P.EXP_MAX:
        assert cmax * bound * 2.0 ** e < 2.0 ** 62                   # cannot overflow ...
        assert cmax * bound * 2.0 ** (e + 2) >= 2.0 ** 62            # ... and wastes at most one bit beyond the safety factor


def test_exponent_bound_never_exceeds_the_formula():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        cmax = int(rng.integers(1, 1 << 34))
        bound = float(2.0 ** rng.uniform(-60, 60))
        e = P.plastic_exponent_bound(cmax, bound)
        formula = 62 - math.ceil(math.log2(cmax * bound))
        assert formula - 1 <= e <= formula


def test_exponent_bound_refuses_non_finite():
    for b in (float('inf'), float('nan')):
        with pytest.raises(ValueError):
            P.plastic_exponent_bound(3, b)


# ------------------------------------------------------------------------------------------------------------ arguments
def test_bounds_are_normalised():
    assert P.plastic_bounds((0, 1)) == (0.0, 1.0)
    assert P.plastic_bounds([np.float32(-0.5), np.array([2.0])]) == (-0.5, 2.0)
    assert P.plastic_bounds((torch.tensor(0.25), 0.25)) == (0.25, 0.25)       # a host tensor is a host number


@pytest.mark.parametrize('bad', [(None, 1.0), (0.0, None), (None, None), (1.0, 0.0), (0.0, float('inf')), (float('nan'), 1.0),
                                 (0.0,), (0.0, 1.0, 2.0), 1.0, 'ab', (np.zeros(2), 1.0), (True, 1.0)])
def test_bad_bounds_are_refused(bad):
    with pytest.raises(ValueError):
        P.plastic_bounds(bad)


def test_device_tensor_bounds_are_refused():
    dev_like = torch.empty((), device='meta')           # any tensor that does not live on the host
    with pytest.raises(ValueError, match='host numbers'):
        P.plastic_bounds((dev_like, 1.0))
    with pytest.raises(ValueError, match='host numbers'):
        P.plastic_bounds((0.0, dev_like))


def test_release_raw_is_refused_before_any_device_work():
    M = object.__new__(be.CSR)                           # no arrays at all: the check comes first
    with pytest.raises(ValueError, match='release_raw'):
        be.CSR.prepare(M, plastic=(0.0, 1.0), release_raw=True)


def test_bad_bounds_are_refused_before_any_device_work():
    for cls in (be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost):
        M = object.__new__(cls)
        M.buffers = {}
        with pytest.raises(ValueError):
            M.prepare(plastic=(1.0, 0.0))
        assert M.plastic_state is None


# ------------------------------------------------------------------------------------------------------------ the header
@pytest.mark.parametrize('name, n_args', [('be_scatter_plan_refresh_workspace_bytes', 1), ('be_scatter_plan_refresh_rows', 20),
                                          ('be_scatter_plan_slots', 16), ('be_scatter_plan_patch_entries', 21)])
def test_header_declares_the_new_symbols(name, n_args):
    text = HEADER.read_text()
    m = re.search(r'\b(?:int|int64_t)\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, re.S)
    assert m, f"{name} is not declared in {HEADER.name}"
    assert len(m.group(1).split(',')) == n_args
