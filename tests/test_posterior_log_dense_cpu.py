"""The C-ABI surface and the Python front of the posteriors' dense log-space route (torbi_hip_forward_backward_log*,
torbi_amd.forward_backward_log, state_posteriors(route='log-dense')) without a device."""
import os
import re

import pytest
import torch

import torbi_amd
from torbi_amd import _lib

NAMES = ('torbi_hip_forward_backward_log_covers', 'torbi_hip_forward_backward_log_workspace_size',
         'torbi_hip_forward_backward_log_tile', 'torbi_hip_forward_backward_log')


def test_symbols_header_and_exports():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, 'torbi_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and callable(getattr(lib, name)) and re.search(rf'\b{name}\(', header)
        assert not name.endswith('_bytes')
    assert lib.torbi_hip_abi_version() == _lib.ABI_VERSION == 17
    for name in ('forward_backward_log', 'forward_backward_log_workspace_bytes'):
        assert callable(getattr(torbi_amd, name)) and name not in torbi_amd.__all__


@pytest.mark.parametrize('case,want', [((1, 1, 1), 1), ((4, 10, 4096), 1), ((512, 500, 1440), 1), ((4, 10, 4097), 0),
                                       ((0, 10, 64), 0), ((4, 0, 64), 0), ((4, 10, 0), 0)])
def test_covers_answers_without_a_device(case, want):
    assert _lib.load().torbi_hip_forward_backward_log_covers(*case, -1) == want


def test_workspace_size_is_the_sum_of_its_parts():
    need = _lib.load().torbi_hip_forward_backward_log_workspace_size
    by_states = [need(8, 60, S) for S in (37, 64, 65, 1440, 4096)]
    by_batch = [need(B, 60, 1440) for B in (1, 8, 64, 512)]
    assert all(n > 256 and n % 256 == 0 for n in by_states + by_batch)
    assert by_states[0] == by_states[1] and by_states[1:] == sorted(set(by_states[1:])) and by_batch == sorted(set(by_batch))
    assert need(8, 60, 1440) == need(8, 1, 1440) == torbi_amd.forward_backward_log_workspace_bytes(8, 500, 1440)
    # 1440 states pad to 1472: both packs, y and the two planes of r, the fp64 sums (64 bytes, a region of 256), the base
    assert need(8, 60, 1440) == 2 * 1472 * 1472 * 4 + 8 * 1472 * 4 + 2 * 8 * 1472 * 4 + 256 + 256
    assert need(0, 60, 1440) == need(8, 60, 4097) == 256


def test_the_route_is_its_own_value_of_route():
    obs, trans = torch.rand(2, 3, 64).softmax(2), torch.rand(64, 64).softmax(1)
    with pytest.raises(RuntimeError, match='needs a HIP device: gpu=None is the float64 route'):
        torbi_amd.state_posteriors(obs, transition=trans, gpu=None, route='log-dense')
    with pytest.raises(RuntimeError, match='there is no transition matrix'):
        torbi_amd.state_posteriors(obs, gpu=0, route='log-dense')
    with pytest.raises(RuntimeError, match="arithmetic must be 'scaled' or 'log'"):
        torbi_amd.state_posteriors(obs, transition=trans, gpu=0, route='log-dense', arithmetic='exact')
    with pytest.raises(RuntimeError, match='route must be'):
        torbi_amd.state_posteriors(obs, transition=trans, gpu=0, route='log-densee')
