"""The C-ABI surface, the Python front and the routing of the log-space band route of path sampling
(torbi_hip_sample_log_band*, forward_sample_log_banded, sample_paths(route='log-band')) without a device."""
import ctypes
import math

import pytest
import torch

import torbi_amd
from torbi_amd import _lib, inputs, sampling, viterbi

NINF = -math.inf
EINVAL, EWORKSPACE = -1, -2                                 # include/torbi_hip.h
G = torch.Generator().manual_seed(1)
OBS, A = torch.softmax(torch.randn(2, 4, 72, generator=G), 2), torch.softmax(torch.randn(72, 72, generator=G), 0)


def test_symbols_and_exports():
    lib = _lib.load()
    for name in ('torbi_hip_sample_log_band_covers', 'torbi_hip_sample_log_band_workspace_size', 'torbi_hip_sample_log_band'):
        wide = name.replace('_log', '_wide')                                    # the arguments are the wide entry's
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[wide] and getattr(lib, name).argtypes == _lib.SYMBOLS[name][1], name
    for name in ('forward_sample_log_banded', 'forward_sample_log_banded_workspace_bytes'):
        assert getattr(torbi_amd, name) is getattr(sampling, name) and name not in torbi_amd.__all__


# (B, T, S, N, reach_left, reach_right, background)
@pytest.mark.parametrize('call,want', [
    ((4, 10, 4096, 4096, 255, 256, NINF), 1), ((4, 10, 4096, 1, 256, 256, NINF), 0),          # W = 512, 513
    ((4, 10, 4097, 1, 8, 8, NINF), 0), ((4, 10, 1440, 0, 87, 87, NINF), 0), ((4, 10, 1440, 4097, 87, 87, NINF), 0),     # S, N
    ((4, 10, 1440, 1, 87, 87, -20.), 0), ((4, 10, 1440, 1, 87, 87, math.nan), 0), ((4, 10, 1440, 1, 87, 87, math.inf), 0),
    ((4, 10, 1440, 1, -1, 87, NINF), 0), ((4, 10, 1440, 1, 87, -1, NINF), 0),                 # a negative reach
    ((3, 12, 64, 1, 2, 5, NINF), 1), ((512, 500, 1440, 16, 87, 87, NINF), 1)])                # a narrow band; the pitch matrix
def test_covers(call, want):
    assert _lib.load().torbi_hip_sample_log_band_covers(*call, -1) == want


@pytest.mark.parametrize('B,T,S,reach', [(8, 60, 1440, 87), (3, 7, 1441, 87), (2, 5, 257, 40)])
def test_workspace_size(B, T, S, reach):
    log = _lib.load().torbi_hip_forward_backward_log_band_workspace_size(B, T, S, reach, reach)
    want = log + (4 * B * T * ((S + 3) // 4 * 4) + 255) // 256 * 256
    for draws in (1, 4096):
        assert torbi_amd.forward_sample_log_banded_workspace_bytes(B, T, S, draws, reach, reach) == want


def test_error_codes_come_before_any_device_call():           # (no device here: reaching for one returns a HIP error)
    B, T, S, N, reach = 2, 3, 128, 2, 40
    need = torbi_amd.forward_sample_log_banded_workspace_bytes(B, T, S, N, reach, reach)
    room = ctypes.create_string_buffer(64)
    p = ctypes.addressof(room)
    call = lambda obs=p, left=reach, size=need, draws=N: _lib.load().torbi_hip_sample_log_band(
        obs, p, p, p, left, reach, NINF, p, p, p, p, size, B, T, S, draws, -1, None)
    assert (call(obs=None), call(left=-1), call(draws=0), call(size=need - 1)) == (EINVAL, EINVAL, EINVAL, EWORKSPACE)


def test_refusals_come_before_a_device_is_asked_for(monkeypatch):
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: pytest.fail('a device was asked for'))
    with pytest.raises(RuntimeError, match='forward_sample_wide_banded.*gpu=None'):       # a finite background
        torbi_amd.forward_sample_log_banded(OBS, None, A, A[0], torch.rand(2, 1, 4), 2, 2, -20.)
    with pytest.raises(RuntimeError, match="route='log-band'.*gpu=None"):
        torbi_amd.sample_paths(OBS, 3, transition=A, gpu=None, route='log-band')
    with pytest.raises(RuntimeError, match="route='log-band'.*no transition matrix"):
        torbi_amd.sample_paths(OBS, 3, gpu=0, route='log-band')
    with pytest.raises(RuntimeError, match='route must be'):
        torbi_amd.sample_paths(OBS, 3, transition=A, gpu=0, route='banded')


@pytest.mark.parametrize('over,reason', [((1, 2, -20.), 'turns down'), (None, 'does not hold one value outside a band')])
def test_sample_paths_raises_where_the_matrix_has_no_minus_inf_band(monkeypatch, over, reason):
    monkeypatch.setattr(viterbi, 'band_over', lambda *args: over)
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: torch.device('cpu'))
    for runner in ('_run', '_run_band', '_run_wide_band', '_run_log_band'):
        monkeypatch.setattr(sampling, runner, lambda *args: pytest.fail('a route ran'))
    with pytest.raises(RuntimeError, match=f"sample_paths\\(route='log-band'\\).*{reason}.*gpu=None"):
        torbi_amd.sample_paths(OBS, 3, transition=A, gpu=0, route='log-band')
