"""The C-ABI surface, the Python front and the routing of the wide band route of path sampling
(torbi_hip_sample_wide_band*, forward_sample_wide_banded, sample_paths(route=)) without a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, band_route, inputs, sampling, viterbi

NINF = -math.inf
TINY = float(np.log(np.finfo(np.float32).tiny))
EINVAL, EWORKSPACE = -1, -2                                 # include/torbi_hip.h


def test_symbols_and_exports():
    lib = _lib.load()
    for name in ('torbi_hip_sample_wide_band_covers', 'torbi_hip_sample_wide_band_workspace_size', 'torbi_hip_sample_wide_band'):
        narrow = name.replace('_wide', '').replace('_size', '_bytes')           # the arguments are the narrow entry's
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[narrow] and getattr(lib, name).argtypes == _lib.SYMBOLS[name][1], name
    for name in ('forward_sample_wide_banded', 'forward_sample_wide_banded_workspace_bytes'):
        assert getattr(torbi_amd, name) is getattr(sampling, name)


# (B, T, S, N, reach_left, reach_right, background)
@pytest.mark.parametrize('call,want', [
    ((512, 500, 1440, 16, 87, 87, NINF), 1), ((512, 500, 1440, 1, 87, 87, TINY), 1),
    ((4, 10, 4096, 4096, 255, 256, NINF), 1), ((4, 10, 4096, 1, 256, 256, NINF), 0),          # W = 512, 513; S = 4096
    ((4, 10, 4097, 1, 8, 8, NINF), 0),                                                        # S = 4097
    ((4, 10, 1440, 0, 87, 87, NINF), 0), ((4, 10, 1440, 4097, 87, 87, NINF), 0),              # N = 0, 4097
    ((4, 10, 1440, 1, 87, 87, math.nan), 0), ((4, 10, 1440, 1, 87, 87, math.inf), 0),
    ((3, 12, 64, 1, 2, 5, NINF), 1)])                                                         # a narrow band
def test_covers(call, want):
    assert _lib.load().torbi_hip_sample_wide_band_covers(*call, -1) == want


@pytest.mark.parametrize('B,T,S,reach', [(8, 60, 1440, 87), (3, 7, 1441, 87), (2, 5, 257, 40)])
def test_workspace_size(B, T, S, reach):
    """The wide posterior's layout (a multiple of 256), then the filter rows (B, T, S4) fp32, whatever the draws."""
    wide = _lib.load().torbi_hip_forward_backward_wide_band_workspace_size(B, T, S, reach, reach)
    want = wide + (4 * B * T * ((S + 3) // 4 * 4) + 255) // 256 * 256
    assert wide % 256 == 0
    for draws in (1, 4096):
        assert torbi_amd.forward_sample_wide_banded_workspace_bytes(B, T, S, draws, reach, reach) == want


def test_error_codes_come_before_any_device_call():
    """There is no device here: a call that reached for one would return a HIP error, not these codes."""
    B, T, S, N, reach = 2, 3, 128, 2, 40
    need = torbi_amd.forward_sample_wide_banded_workspace_bytes(B, T, S, N, reach, reach)
    room = ctypes.create_string_buffer(64)
    p = ctypes.addressof(room)
    call = lambda obs=p, left=reach, size=need: _lib.load().torbi_hip_sample_wide_band(
        obs, p, p, p, left, reach, NINF, p, p, p, p, size, B, T, S, N, -1, None)
    assert (call(obs=None), call(left=-1), call(size=need - 1)) == (EINVAL, EINVAL, EWORKSPACE)


@pytest.mark.parametrize('route', band_route.ROUTES)
@pytest.mark.parametrize('band,runner', [((40, 30, -20.), 'wide'), ((1, 2, -20.), 'narrow')])
def test_routing(monkeypatch, route, band, runner):
    """A band only the wide route covers reaches the wide runner under 'band' and is None under 'dense'; a narrow band still
    reaches `_run_band`; one look at the matrix."""
    looks = []
    monkeypatch.setattr(viterbi, 'band_over', lambda *args: looks.append(args) or band)
    monkeypatch.setattr(sampling, '_covered', lambda *args: runner == 'narrow')
    monkeypatch.setattr(sampling, '_wide_covered', lambda *args: True)
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: torch.device('cpu'))
    monkeypatch.setattr(sampling, '_run', lambda *args: 'dense')
    monkeypatch.setattr(sampling, '_run_band', lambda *args: ('narrow',) + args[-3:])
    monkeypatch.setattr(sampling, '_run_wide_band', lambda *args: ('wide',) + args[-3:])
    g = torch.Generator().manual_seed(1)
    obs, A = torch.softmax(torch.randn(2, 4, 72, generator=g), 2), torch.softmax(torch.randn(72, 72, generator=g), 0)
    got = torbi_amd.sample_paths(obs, 3, transition=A, gpu=0, route=route)
    if route == 'dense':
        assert got == 'dense' and not looks and sampling._band_run('dense', A, A, 2, 4, 72, 3, 0) is None
        return
    pays = (sampling._wide_band_pays if runner == 'wide' else sampling._band_pays)(2, 72, *band[:2], 3)
    assert got == ((runner,) + band if route == 'band' or pays else 'dense') and len(looks) == 1
    assert torbi_amd.sample_route(A, 2, 4, 72, draws=3, gpu=0) == ('band' if pays else 'dense')

