"""The C-ABI surface, the Python front and the `arithmetic=` keyword of the log-space band route of path entropy
(torbi_hip_path_entropy_log_band*, entropy.forward_entropy_log_banded, entropy.path_entropy(arithmetic=)) without a device."""
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, entropy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -math.inf
TINY = float(np.log(np.finfo(np.float32).tiny))
NAMES = ('torbi_hip_path_entropy_log_band_covers', 'torbi_hip_path_entropy_log_band_workspace_size',
         'torbi_hip_path_entropy_log_band_tile', 'torbi_hip_path_entropy_log_band')


def test_symbols_and_exports():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    assert lib.torbi_hip_abi_version() == _lib.ABI_VERSION == 17
    for name in NAMES:
        assert re.search(r'\b(?:int|size_t) ' + name + r'\s*\(', header), name
        assert name in _lib.SYMBOLS and callable(getattr(lib, name)) and not name.endswith('_bytes')
    for name in ('forward_entropy_log_banded', 'path_entropy_log_banded_workspace_bytes'):
        assert name in entropy.__all__ and callable(getattr(entropy, name))
        assert name not in torbi_amd.__all__ and not hasattr(torbi_amd, name)


@pytest.mark.parametrize('case,want', [
    ((512, 500, 1440, 87, 87, NINF), 1), ((3, 12, 64, 2, 5, NINF), 1), ((3, 5, 37, 1000, 1000, NINF), 1),
    ((4, 10, 4096, 255, 256, NINF), 1), ((4, 10, 4096, 256, 256, NINF), 0),              # W = 512 and 513
    ((4, 10, 4097, 8, 8, NINF), 0),                                                          # S = 4097
    ((512, 500, 1440, 87, 87, TINY), 0), ((3, 12, 64, 2, 5, -3.0), 0), ((4, 10, 1440, 87, 87, math.nan), 0),
    ((4, 10, 1440, 87, 87, math.inf), 0), ((4, 10, 1440, -1, 87, NINF), 0), ((0, 10, 1440, 87, 87, NINF), 0)])
def test_covers(case, want):
    lib = _lib.load()
    assert lib.torbi_hip_path_entropy_log_band_covers(*case, -1) == want
    if case[5] == NINF:
        assert lib.torbi_hip_forward_backward_counts_log_band_covers(*case, -1) == want


def test_workspace_size():
    need = _lib.load().torbi_hip_path_entropy_log_band_workspace_size
    sizes = [need(8, 60, 1440, reach, reach) for reach in (11, 40, 87, 255)]
    assert all(n > 0 and n % 256 == 0 for n in sizes) and sizes == sorted(set(sizes))
    assert sizes[2] == entropy.path_entropy_log_banded_workspace_bytes(8, 60, 1440, 87, 87)
    # the forward pack of 6 blocks x 44 dquads x 4 KiB; the prefix of 8 x 60 floats up to 256 bytes; the flag; room to align
    # the base
    assert sizes[2] == 6 * 44 * 4096 + 2048 + 256 + 256
    for bad in ((0, 60, 1440, 87, 87), (8, 0, 1440, 87, 87), (8, 60, 4097, 87, 87), (8, 60, 1440, -1, 87), (8, 60, 1440, 87, -1)):
        assert need(*bad) == 256


def test_arithmetic_is_checked_first_and_ignored_on_the_host():
    g = torch.Generator().manual_seed(3)
    obs, A = torch.softmax(torch.randn(2, 5, 8, generator=g), 2), torch.softmax(torch.randn(8, 8, generator=g), 0)
    with pytest.raises(RuntimeError, match="arithmetic must be 'scaled' or 'log'"):
        entropy.path_entropy(obs[0], transition=A, gpu=None, arithmetic='exact')     # (before the shape is looked at)
    scaled = entropy.path_entropy(obs, transition=A, gpu=None, prefix=True)
    logs = entropy.path_entropy(obs, transition=A, gpu=None, prefix=True, arithmetic='log')
    assert all(torch.equal(a, b) for a, b in zip(scaled, logs))
    for model, route in ((A, 'dense'), (None, 'auto')):                               # raised before a device is asked for
        with pytest.raises(RuntimeError, match='band route only.*gpu=None'):
            entropy.path_entropy(obs, transition=model, gpu=0, route=route, arithmetic='log')
