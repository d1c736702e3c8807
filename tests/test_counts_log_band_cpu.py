"""What the log-space band counts (csrc/counts_log_band.hpp, torbi_amd.forward_backward_counts_log_banded, `arithmetic=` of
expected_counts and log_likelihood) answer without a device."""
import math
import os
import re

import pytest
import torch

import torbi_amd
from torbi_amd import _lib

NINF = -math.inf
NAMES = tuple('torbi_hip_forward_backward_counts_log_band' + tail for tail in ('', '_covers', '_workspace_size', '_shares'))
up = lambda n, to: -(-n // to) * to


def test_symbols_header_and_exports():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, 'torbi_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and callable(getattr(lib, name)) and re.search(rf'\b{name}\(', header)
    assert lib.torbi_hip_abi_version() == _lib.ABI_VERSION == 17
    for name in ('forward_backward_counts_log_banded', 'expected_counts_log_banded_workspace_bytes'):
        assert callable(getattr(torbi_amd, name))


@pytest.mark.parametrize('case,want', [((4, 10, 4096, 255, 256, NINF), 1), ((4, 10, 4096, 256, 256, NINF), 0),
                                       ((4, 10, 4097, 8, 8, NINF), 0), ((4, 10, 1440, 87, 87, math.nan), 0)])
def test_covers_what_the_log_posterior_route_covers(case, want):
    lib = _lib.load()
    assert (lib.torbi_hip_forward_backward_counts_log_band_covers(*case, -1) == want
            == lib.torbi_hip_forward_backward_log_band_covers(*case, -1))


def test_workspace_size_is_the_documented_layout():
    lib = _lib.load()
    B, T, S, left, right = 8, 60, 1440, 87, 87
    W, S4 = left + right + 1, up(S, 4)
    # 175 diagonals: 2 chunks of 4 x 24; 23 blocks of 64 next states; 480 K rows are 30 blocks of 16:
    # min(64, 30, ceil(1024 / 46)) = 23 shares wanted, so 2 blocks a share and 15 shares
    blocks = -(-B * T // 16)
    want = min(64, blocks, -(-1024 // (-(-S // 64) * 2)))
    shares = -(-blocks // -(-blocks // want))
    assert shares == 15 == lib.torbi_hip_forward_backward_counts_log_band_shares(B, T, S, left, right)
    log = lib.torbi_hip_forward_backward_log_band_workspace_size(B, T, S, left, right)
    need = log + 2 * up(4 * B * T * S4, 256) + up(4 * B * T, 256) + up(4 * shares * S * W, 256)
    assert torbi_amd.expected_counts_log_banded_workspace_bytes(B, T, S, left, right) == need
    for bad in ((0, T, S, left, right), (B, T, 4097, left, right), (B, T, S, -1, right)):
        assert lib.torbi_hip_forward_backward_counts_log_band_workspace_size(*bad) == 256
        assert lib.torbi_hip_forward_backward_counts_log_band_shares(*bad) == 0


def test_arithmetic_is_checked_before_anything_runs():
    obs, trans = torch.rand(2, 3, 64).softmax(2), torch.rand(64, 64).softmax(1)
    init = torch.full((64,), 1 / 64)
    for call in (lambda **kw: torbi_amd.expected_counts(obs, transition=trans, gpu=0, **kw),
                 lambda **kw: torbi_amd.log_likelihood(obs.log(), None, trans.log(), init.log(), **kw)):
        with pytest.raises(RuntimeError, match="arithmetic must be 'scaled' or 'log'"):
            call(arithmetic='exact')
    with pytest.raises(RuntimeError, match='log arithmetic has a band route only.*gpu=None'):
        torbi_amd.expected_counts(obs, transition=trans, gpu=0, route='dense', arithmetic='log')
    with pytest.raises(RuntimeError, match='log arithmetic has a band route only.*gpu=None'):
        torbi_amd.expected_counts(obs, gpu=0, route='band', arithmetic='log')
    X = torbi_amd.expected_counts(obs, transition=trans, gpu=None, arithmetic='log')[0]          # the host route ignores it
    assert torch.equal(X, torbi_amd.expected_counts(obs, transition=trans, gpu=None)[0])
    L = torbi_amd.log_likelihood(obs.log(), None, trans.log(), init.log(), route='dense', arithmetic='log')   # CPU tensors too
    assert torch.equal(L, torbi_amd.log_likelihood(obs.log(), None, trans.log(), init.log()))
