"""The C-ABI surface and the Python front of the posteriors' band route (torbi_hip_forward_backward_band*,
torbi_amd.forward_backward_banded) without a device."""
import ctypes
import math
import os
import re

import pytest
import torch

import torbi_amd
from torbi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('torbi_hip_forward_backward_band_covers', 'torbi_hip_forward_backward_band_workspace_bytes',
         'torbi_hip_forward_backward_band')


def test_symbols_are_declared_and_exported_within_abi_17():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf'\b{name}\s*\(', header) and name in _lib.SYMBOLS and hasattr(lib, name)
    assert '#define TORBI_HIP_ABI_VERSION 17' in header and _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    for name in ('forward_backward_banded', 'forward_backward_banded_workspace_bytes', 'posterior_route'):
        assert name in torbi_amd.__all__ and callable(getattr(torbi_amd, name))


def test_covers_answers_without_a_device():
    covers = _lib.load().torbi_hip_forward_backward_band_covers
    f = ctypes.c_float
    assert covers(512, 500, 1440, 11, 11, f(-math.inf), 0) == 1
    assert covers(512, 500, 1440, 11, 11, f(-87.33654), 0) == 1
    assert covers(4, 10, 4096, 31, 32, f(-math.inf), 0) == 1                 # W = 64
    assert covers(4, 10, 4096, 32, 32, f(-math.inf), 0) == 0                 # W = 65
    assert covers(4, 10, 1440, 64, 0, f(-math.inf), 0) == 0                  # ... on one side
    assert covers(4, 10, 4097, 11, 11, f(-math.inf), 0) == 0
    assert covers(4, 10, 1440, 11, 11, f(math.nan), 0) == 0
    assert covers(4, 10, 1440, 11, 11, f(math.inf), 0) == 0
    assert covers(4, 10, 1440, -1, 11, f(-math.inf), 0) == 0
    assert covers(0, 10, 1440, 11, 11, f(-math.inf), 0) == 0
    # a band wider than the matrix is clipped: a matrix row holds min(W, S) entries
    assert covers(9, 12, 37, 36, 36, f(-3.0), 0) == 1
    assert covers(9, 12, 64, 1000, 1000, f(-3.0), 0) == 1
    assert covers(9, 12, 65, 64, 64, f(-3.0), 0) == 0


def test_workspace_bytes_grow_with_the_band():
    need = _lib.load().torbi_hip_forward_backward_band_workspace_bytes
    sizes = [need(8, 60, 1440, r, r) for r in (0, 1, 11, 31)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))
    assert need(8, 60, 1440, 11, 11) == torbi_amd.forward_backward_banded_workspace_bytes(8, 60, 1440, 11, 11)
    assert need(9, 60, 1440, 11, 11) > need(8, 60, 1440, 11, 11)
    assert need(9, 12, 37, 36, 36) == need(9, 12, 37, 1000, 1000)            # reaches beyond S - 1 are clamped


def test_c_abi_argument_errors_without_a_device():
    lib = _lib.load()
    B, T, S, left, right = 3, 5, 7, 1, 2
    need = lib.torbi_hip_forward_backward_band_workspace_bytes(B, T, S, left, right)
    p = ctypes.c_void_p(16)                  # never dereferenced: every call below fails its argument check first
    s = ctypes.c_void_p(0)
    bg = ctypes.c_float(-math.inf)
    call = lib.torbi_hip_forward_backward_band
    assert call(p, p, p, p, left, right, bg, p, p, p, need - 1, B, T, S, 0, s) == -2           # TORBI_HIP_EWORKSPACE
    assert call(p, p, p, p, left, right, bg, p, p, p, need, B, 0, S, 0, s) == -1               # T < 1
    assert call(p, p, p, p, left, right, bg, p, p, p, need, B, T, 0, 0, s) == -1               # S < 1
    assert call(p, p, p, p, left, right, bg, p, p, p, need, -1, T, S, 0, s) == -1              # B < 0
    assert call(p, p, p, p, -1, right, bg, p, p, p, need, B, T, S, 0, s) == -1                 # negative reach
    for hole in (0, 1, 2, 3, 7, 8, 9):                                                         # a null pointer
        args = [p, p, p, p, left, right, bg, p, p, p, need, B, T, S, 0, s]
        args[hole] = None
        assert call(*args) == -1
    assert call(p, p, p, p, left, right, bg, p, p, p, 1 << 40, B, T, 20000, 0, s) == -3        # S beyond the build
    assert call(p, p, p, p, left, right, bg, p, p, p, 1 << 40, B, T, 5000, 0, s) == -5         # ... beyond the band route
    assert call(p, p, p, p, 40, 40, bg, p, p, p, 1 << 40, B, T, 1440, 0, s) == -5              # W = 81
    assert call(p, p, p, p, left, right, ctypes.c_float(math.nan), p, p, p, need, B, T, S, 0, s) == -5
    assert call(None, None, None, None, left, right, bg, None, None, None, 0, 0, T, S, 0, s) == 0   # B = 0: nothing to do


def test_misshaped_inputs_raise_before_any_work():
    B, T, S = 3, 4, 5
    obs = torch.zeros((B, T, S))
    trans, init = torch.zeros((S, S)), torch.zeros(S)
    frames = torch.full((B,), T, dtype=torch.int32)
    bad = [(dict(batch_frames=torch.tensor([5], dtype=torch.int32)), r'batch_frames must have shape \(3,\)'),
           (dict(initial=torch.zeros(1)), r'initial must have shape \(5,\)'),
           (dict(transition=torch.zeros((S - 1, S - 1))), r'transition must have shape \(5, 5\)'),
           (dict(transition=torch.zeros((S, S - 1))), 'transition must have shape'),
           (dict(transition=None), 'needs a transition matrix'),
           (dict(reach_left=-1), 'must be >= 0'),
           (dict(background=math.inf), 'does not cover')]
    for change, message in bad:
        args = dict(batch_frames=frames, transition=trans, initial=init, reach_left=1, reach_right=1)
        args.update(change)
        with pytest.raises(RuntimeError, match=message):
            torbi_amd.forward_backward_banded(obs, **args)
    with pytest.raises(RuntimeError, match='observation must have shape'):
        torbi_amd.forward_backward_banded(obs[0], frames, trans, init, 1, 1)
    with pytest.raises(RuntimeError, match='route must be'):
        torbi_amd.state_posteriors(obs, frames, trans, init, log_probs=True, gpu=None, route='banded')
    assert torbi_amd.posterior_route(None, B, T, S) == 'uniform'
    with pytest.raises(RuntimeError, match='transition must have shape'):
        torbi_amd.posterior_route(torch.zeros((S, S - 1)), B, T, S)
