"""What the wide band counts route (csrc/counts_wide_band.hpp, torbi_amd.forward_backward_counts_wide_banded) answers without a
device."""
import math

import pytest

import torbi_amd
from torbi_amd import _lib

NINF = -math.inf
up = lambda n, to: -(-n // to) * to


def test_names():
    for name in ('forward_backward_counts_wide_banded', 'expected_counts_wide_banded_workspace_bytes'):
        assert callable(getattr(torbi_amd, name)) and name not in torbi_amd.__all__


def test_workspace_size_is_the_documented_layout():
    lib = _lib.load()
    B, T, S, left, right = 8, 60, 1440, 87, 87
    W, S4 = left + right + 1, up(S, 4)
    # 23 blocks of 64 next states x 1 window chunk; 480 K rows are 8 blocks of 64: min(64, 8, ceil(1024 / 23)) = 8 shares of one
    blocks = -(-B * T // 64)
    want = min(64, blocks, -(-1024 // (-(-S // 64) * -(-(W + 66) // 256))))
    shares = -(-blocks // -(-blocks // want))
    assert shares == 8 == lib.torbi_hip_forward_backward_counts_wide_band_shares(B, T, S, left, right)
    wide = lib.torbi_hip_forward_backward_wide_band_workspace_size(B, T, S, left, right)
    need = wide + 2 * up(4 * B * T * S4, 256) + up(4 * shares * S * W, 256)
    assert torbi_amd.expected_counts_wide_banded_workspace_bytes(B, T, S, left, right) == need
    for bad in ((0, T, S, left, right), (B, 0, S, left, right), (B, T, 4097, left, right), (B, T, S, -1, right)):
        assert lib.torbi_hip_forward_backward_counts_wide_band_workspace_size(*bad) == 256
        assert lib.torbi_hip_forward_backward_counts_wide_band_shares(*bad) == 0


@pytest.mark.parametrize('case', [(512, 500, 1440, 87, 87, NINF), (3, 12, 64, 2, 5, NINF), (4, 10, 4096, 255, 256, -3.0),
                                  (4, 10, 4096, 256, 256, NINF), (4, 10, 4097, 8, 8, NINF), (4, 10, 1440, 87, 87, math.nan),
                                  (0, 10, 1440, 87, 87, NINF)])
def test_covers_what_the_wide_posterior_route_covers(case):
    lib = _lib.load()
    assert (lib.torbi_hip_forward_backward_counts_wide_band_covers(*case, -1)
            == lib.torbi_hip_forward_backward_wide_band_covers(*case, -1))
