"""The C-ABI surface and the Python front of the posteriors' wide band route (torbi_hip_forward_backward_wide_band*,
torbi_amd.forward_backward_wide_banded) without a device."""
import math

import numpy as np
import pytest

import torbi_amd
from torbi_amd import _lib

NINF = -math.inf
TINY = float(np.log(np.finfo(np.float32).tiny))
NAMES = ('torbi_hip_forward_backward_wide_band_covers', 'torbi_hip_forward_backward_wide_band_workspace_size',
         'torbi_hip_forward_backward_wide_band')


def test_symbols_and_exports():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SYMBOLS and callable(getattr(lib, name))
    for name in ('forward_backward_wide_banded', 'forward_backward_wide_banded_workspace_bytes'):
        assert callable(getattr(torbi_amd, name))


@pytest.mark.parametrize('case,want', [
    ((512, 500, 1440, 87, 87, NINF), 1), ((512, 500, 1440, 87, 87, TINY), 1), ((4, 10, 4096, 255, 256, NINF), 1),
    ((3, 5, 37, 1000, 1000, -3.0), 1),                                      # clamped to the matrix
    ((3, 12, 64, 2, 5, NINF), 1),                                            # a narrow band: one kernel, not a patch
    ((4, 10, 4096, 256, 256, NINF), 0), ((4, 10, 4097, 8, 8, NINF), 0), ((4, 10, 1440, 87, 87, math.nan), 0),
    ((4, 10, 1440, 87, 87, math.inf), 0), ((4, 10, 1440, -1, 87, NINF), 0), ((4, 10, 1440, 87, -1, NINF), 0),
    ((0, 10, 1440, 87, 87, NINF), 0)])
def test_covers(case, want):
    assert _lib.load().torbi_hip_forward_backward_wide_band_covers(*case, -1) == want


def test_workspace_size():
    need = _lib.load().torbi_hip_forward_backward_wide_band_workspace_size
    sizes = [need(8, 60, 1440, reach, reach) for reach in (11, 40, 87, 255)]
    assert all(n > 0 and n % 256 == 0 for n in sizes) and sizes == sorted(set(sizes))
    assert sizes[2] == torbi_amd.forward_backward_wide_banded_workspace_bytes(8, 60, 1440, 87, 87)
    # both packs of 6 blocks x 44 dquads x 4 KiB, the row maxima and sums, the flag, room to align the base
    assert sizes[2] == 2 * 6 * 44 * 4096 + 2 * 2048 + 256 + 256
