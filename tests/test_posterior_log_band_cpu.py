"""The C-ABI surface and the Python front of the posteriors' log-space band route (torbi_hip_forward_backward_log_band*,
torbi_amd.forward_backward_log_banded, state_posteriors(arithmetic=)) without a device."""
import math
import os
import re

import pytest
import torch

import torbi_amd
from torbi_amd import _lib

NINF = -math.inf
NAMES = ('torbi_hip_forward_backward_log_band_covers', 'torbi_hip_forward_backward_log_band_workspace_size',
         'torbi_hip_forward_backward_log_band_tile', 'torbi_hip_forward_backward_log_band')


def test_symbols_header_and_exports():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, 'torbi_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and callable(getattr(lib, name)) and re.search(rf'\b{name}\(', header)
    assert lib.torbi_hip_abi_version() == _lib.ABI_VERSION == 17
    for name in ('forward_backward_log_banded', 'forward_backward_log_banded_workspace_bytes'):
        assert callable(getattr(torbi_amd, name))


@pytest.mark.parametrize('case,want', [
    ((4, 10, 4096, 255, 256, NINF), 1), ((3, 12, 64, 2, 5, -20.0), 1), ((3, 5, 37, 1000, 1000, -3.0), 1),
    ((4, 10, 4096, 256, 256, NINF), 0), ((4, 10, 4097, 8, 8, NINF), 0), ((4, 10, 1440, 87, 87, math.nan), 0),
    ((4, 10, 1440, 87, 87, math.inf), 0)])
def test_covers_answers_without_a_device(case, want):
    assert _lib.load().torbi_hip_forward_backward_log_band_covers(*case, -1) == want


def test_workspace_size_grows_with_the_band_and_not_with_the_batch():
    need = _lib.load().torbi_hip_forward_backward_log_band_workspace_size
    sizes = [need(8, 60, 1440, reach, reach) for reach in (11, 40, 87, 255)]
    assert all(n > 0 and n % 256 == 0 for n in sizes) and sizes == sorted(set(sizes))
    assert sizes[2] == need(4096, 500, 1440, 87, 87) == torbi_amd.forward_backward_log_banded_workspace_bytes(1, 1, 1440, 87, 87)
    assert sizes[2] == 2 * 6 * 44 * 4096 + 256 + 256          # both packs of 6 blocks x 44 dquads x 4 KiB, the flag, the base


def test_state_posteriors_checks_arithmetic_before_anything_runs():
    obs, trans = torch.rand(2, 3, 64).softmax(2), torch.rand(64, 64).softmax(1)
    with pytest.raises(RuntimeError, match="arithmetic must be 'scaled' or 'log'"):
        torbi_amd.state_posteriors(obs, transition=trans, gpu=0, arithmetic='exact')
    with pytest.raises(RuntimeError, match='log arithmetic has a band route only.*gpu=None'):
        torbi_amd.state_posteriors(obs, transition=trans, gpu=0, route='dense', arithmetic='log')
    g, L = torbi_amd.state_posteriors(obs, transition=trans, gpu=None, arithmetic='log')     # the host route ignores it
    assert torch.equal(g, torbi_amd.state_posteriors(obs, transition=trans, gpu=None)[0])
