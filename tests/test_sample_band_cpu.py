"""The band route of posterior path sampling without a device: the float64 band rule (`sampling._host_banded`) against the
dense rule and against the posteriors, the C-ABI surface of torbi_hip_sample_band* and the Python front (SAMPLING.md,
"Band route")."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import torbi_amd
from torbi_amd import _lib, sampling

import sample_cases as sc
import sample_band_cases as sbc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('torbi_hip_sample_band_covers', 'torbi_hip_sample_band_workspace_bytes', 'torbi_hip_sample_band')
EINVAL, EWORKSPACE, ERANGE, EUNSUPPORTED = -1, -2, -3, -5


def test_names_symbols_and_abi():
    for name in ('forward_sample_banded', 'forward_sample_banded_workspace_bytes', 'sample_route'):
        assert name in torbi_amd.__all__ and callable(getattr(torbi_amd, name))
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    declared = set(re.findall(r'\b(torbi_hip_\w+)\s*\(', header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert '#define TORBI_HIP_ABI_VERSION 17' in header and _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert inspect.signature(torbi_amd.sample_paths).parameters['route'].default == 'dense'
    assert list(inspect.signature(torbi_amd.sample_paths).parameters)[-1] == 'route'


@pytest.mark.parametrize('B,T,S,band,lengths', [(4, 8, 9, (1, 2), (8, 4, 1, 8)), (3, 7, 12, (0, 0), None),
                                                (2, 5, 6, (5, 5), (5, 2)), (3, 6, 10, (3, 0), (6, 1, 4))])
def test_with_minus_inf_outside_the_band_rule_is_the_dense_rule(B, T, S, band, lengths):
    """background = -inf: the second part has weight 0, so indices and L equal `sampling._host` bit for bit."""
    obs, A, pi = sc.problem(B, T, S, seed=B + T + S, band=band)
    frames = sc.frames_of(lengths, B, T)
    u = sc.uniforms(B, 50, T, seed=S)
    u[:, 0] = 0.
    u[:, 1] = 1.
    dense, L = sc.host(obs, frames, A, pi, u)
    banded, Lb = sbc.host(obs, frames, A, pi, u, band, -math.inf)
    assert bool((dense >= 0).all())
    assert torch.equal(banded, dense) and torch.equal(Lb, L)
    assert sbc.pairs_in_band(banded, frames.long(), band)


def test_finite_background_returns_only_states_of_positive_weight():
    B, T, S, band, bg = 3, 7, 10, (2, 1), -3.
    obs, A, pi = sbc.problem(B, T, S, seed=5, band=band, background=bg)
    obs[:, :, 0] = -math.inf
    obs[:, 2, 4] = -math.inf
    pi[1] = -math.inf
    frames = torch.tensor([7, 3, 1], dtype=torch.int32)
    u = sc.uniforms(B, 64, T, seed=5)
    u[:, 0] = 0.
    u[:, 1] = 1.
    u[:, 2] = math.nan
    indices, L = sbc.host(obs, frames, A, pi, u, band, bg)
    a, E, L64, F, _ = sc.reference(obs, frames, A, pi)
    assert torch.equal(L, L64) and bool(torch.isfinite(L).all())
    worst, behind = sbc.draw_errors(indices, u, a, E, F, band, bg)
    assert worst == 0. and behind > 0.                            # the host route IS the rule; both parts are taken
    assert torch.equal(indices[:, 2], indices[:, 0])
    assert bool((indices != 0).all()) and bool((indices[0, :, 2] != 4).all()) and bool((indices[:, :, 0] != 1).all())
    assert sc.tails_repeat(indices, F)
    assert not sbc.pairs_in_band(indices, F, band)               # (a finite background: pairs outside the band are drawn)


@pytest.mark.parametrize('case,seed', [(k, seed) for k, c in enumerate(sbc.FREQUENCY_CASES) for seed in c[6]])
def test_frequencies_follow_the_posteriors(case, seed):
    """|f - p| <= 5 (sqrt(p (1 - p) / N) + 1 / N) for marginals against gamma and pairs against xi of the DENSE model: the
    band rule draws exactly from it.  The host rule alone stays below 4, which is what keeps a seed in the list."""
    B, T, S, band, bg, lengths, _ = sbc.FREQUENCY_CASES[case]
    obs, A, pi = sbc.problem(B, T, S, seed, band, bg)
    frames = sc.frames_of(lengths, B, T)
    u = sc.uniforms(B, sbc.FREQUENCY_DRAWS, T, seed)
    indices, _ = sbc.host(obs, frames, A, pi, u, band, bg)
    a, E, _, F, gamma = sc.reference(obs, frames, A, pi)
    ratio = sc.frequency_ratio(indices, a, E, F, gamma)
    print(f'band frequency ratio case {case} seed {seed}: {ratio:.2f} of 5')
    assert ratio < 4
    assert sc.tails_repeat(indices, F)
    assert sbc.draw_errors(indices, u, a, E, F, band, bg)[0] == 0.
    if bg == -math.inf:
        assert sbc.pairs_in_band(indices, F, band)


def test_host_rule_marks_nonfinite_items_and_a_broken_promise():
    B, T, S, band, bg = 4, 6, 8, (1, 1), -3.
    obs, A, pi = sbc.problem(B, T, S, seed=2, band=band, background=bg)
    frames = torch.tensor([6, 6, 4, 6], dtype=torch.int32)
    u = sc.uniforms(B, 9, T, seed=2)
    clean, cleanL = sbc.host(obs, frames, A, pi, u, band, bg)
    bad = obs.clone()
    bad[1, 3, 2] = math.nan
    bad[2, 5, 0] = math.nan                      # beyond the item's frames: not read
    bad[3, 2, :] = -math.inf                     # a frame of probability 0
    indices, L = sbc.host(bad, frames, A, pi, u, band, bg)
    assert math.isnan(float(L[1])) and float(L[3]) == -math.inf and bool((indices[[1, 3]] == -1).all())
    for b in (0, 2):
        assert torch.equal(indices[b], clean[b]) and float(L[b]) == float(cleanL[b])
    broken = A.clone()
    broken[0, S - 1] = -2.
    indices, L = sbc.host(obs, frames, broken, pi, u, band, bg)
    assert bool(torch.isnan(L).all()) and bool((indices == -1).all())


def test_covers_answers_without_a_device():
    covers = _lib.load().torbi_hip_sample_band_covers
    f = ctypes.c_float
    assert covers(512, 500, 1440, 1, 11, 11, f(-math.inf), 0) == 1
    assert covers(512, 500, 1440, 4096, 11, 11, f(-87.33654), 0) == 1
    assert covers(512, 500, 1440, 0, 11, 11, f(-math.inf), 0) == 0
    assert covers(512, 500, 1440, 4097, 11, 11, f(-math.inf), 0) == 0
    assert covers(4, 10, 4096, 33, 31, 32, f(-math.inf), 0) == 1                 # W = 64
    assert covers(4, 10, 4096, 33, 32, 32, f(-math.inf), 0) == 0                 # W = 65
    assert covers(4, 10, 4097, 33, 11, 11, f(-math.inf), 0) == 0
    assert covers(4, 10, 1440, 33, 11, 11, f(math.nan), 0) == 0
    assert covers(4, 10, 1440, 33, 11, 11, f(math.inf), 0) == 0
    assert covers(4, 10, 1440, 33, -1, 11, f(-math.inf), 0) == 0
    assert covers(9, 12, 37, 33, 36, 36, f(-3.0), 0) == 1                        # a band wider than the matrix is clipped
    for args in ((512, 500, 1440, 11, 11, -math.inf), (4, 10, 4096, 32, 32, -math.inf), (9, 12, 37, 36, 36, -3.),
                 (4, 10, 1440, 11, 11, math.nan)):
        B, T, S, left, right, bg = args
        assert covers(B, T, S, 7, left, right, f(bg), 0) == _lib.load().torbi_hip_forward_backward_band_covers(
            B, T, S, left, right, f(bg), 0)


def test_library_argument_errors_need_no_device():
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                    # never read: every check comes before the device is touched
    big = ctypes.c_size_t(1 << 62)
    names = ('obs', 'frames', 'trans', 'init', 'u', 'out', 'L', 'w')

    def call(B=2, T=5, S=4, N=3, left=1, right=1, bg=-math.inf, ws=big, **null):
        q = {k: None if null.get(k) else p for k in names}
        return lib.torbi_hip_sample_band(q['obs'], q['frames'], q['trans'], q['init'], left, right, ctypes.c_float(bg), q['u'],
                                         q['out'], q['L'], q['w'], ws, B, T, S, N, 0, None)

    for name in names:
        assert call(**{name: True}) == EINVAL, name
    assert call(left=-1) == EINVAL and call(right=-1) == EINVAL
    assert call(N=0) == EINVAL and call(N=4097) == EINVAL and call(T=0) == EINVAL and call(S=0) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(S=1440, left=40, right=40) == EUNSUPPORTED                      # W = 81 at S > 64
    assert call(S=4097) == EUNSUPPORTED
    assert call(bg=math.nan) == EUNSUPPORTED and call(bg=math.inf) == EUNSUPPORTED
    assert call(S=16385) == ERANGE
    assert call(B=1 << 20, T=2, N=4096) == ERANGE                               # B * N * T = 2^33
    assert call(ws=ctypes.c_size_t(256)) == EWORKSPACE
    need = lib.torbi_hip_sample_band_workspace_bytes(2, 5, 4, 3, 1, 1)
    assert call(ws=ctypes.c_size_t(need - 1)) == EWORKSPACE
    assert lib.torbi_hip_sample_band(None, None, None, None, 1, 1, ctypes.c_float(-math.inf), None, None, None, None,
                                     ctypes.c_size_t(0), 0, 5, 4, 3, 0, None) == 0            # B = 0: nothing to do


@pytest.mark.parametrize('B,T,S,N,left,right', [(1, 1, 8, 1, 1, 1), (4, 20, 1440, 16, 11, 11), (5, 30, 1441, 33, 12, 12),
                                                (70, 6, 257, 4096, 3, 0), (9, 12, 37, 33, 36, 36)])
def test_workspace_bytes_follow_the_stated_layout(B, T, S, N, left, right):
    """forward_backward_banded's workspace, then the filter rows (B, T, S) float32 on the next 256-byte boundary; whatever
    the draws, and without a device."""
    def up(x):
        return (x + 255) // 256 * 256
    need = torbi_amd.forward_sample_banded_workspace_bytes(B, T, S, N, left, right)
    assert need == torbi_amd.forward_backward_banded_workspace_bytes(B, T, S, left, right) + up(4 * B * T * S)
    assert need == torbi_amd.forward_sample_banded_workspace_bytes(B, T, S, 1, left, right)


def test_python_argument_errors_come_before_anything_runs():
    obs, A, pi = sc.problem(2, 5, 4, seed=1, band=(1, 1))
    u = torch.rand(2, 3, 5)
    banded = torbi_amd.forward_sample_banded
    with pytest.raises(RuntimeError, match='transition matrix'):
        banded(obs, None, None, pi, u, 1, 1)
    for wrong in (torch.rand(2, 3, 4), torch.rand(3, 3, 5), torch.rand(2, 5), torch.rand(2, 5000, 5)):
        with pytest.raises(RuntimeError, match='uniforms must have shape|draws must be'):
            banded(obs, None, A, pi, wrong, 1, 1)
    with pytest.raises(RuntimeError, match='batch_frames must have shape'):
        banded(obs, torch.tensor([5, 5, 5]), A, pi, u, 1, 1)
    with pytest.raises(RuntimeError, match='transition must have shape'):
        banded(obs, None, A[:3], pi, u, 1, 1)
    with pytest.raises(RuntimeError, match='initial must have shape'):
        banded(obs, None, A, pi[:3], u, 1, 1)
    with pytest.raises(RuntimeError, match='must be >= 0'):
        banded(obs, None, A, pi, u, -1, 1)
    with pytest.raises(RuntimeError, match='does not cover'):
        banded(obs, None, A, pi, u, 1, 1, background=math.inf)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='HIP device'):
            banded(obs, None, A, pi, u, 1, 1)
    args = dict(draws=3, transition=A, initial=pi, log_probs=True, uniforms=u)
    with pytest.raises(RuntimeError, match='route must be'):
        torbi_amd.sample_paths(obs, route='banded', **args)
    with pytest.raises(RuntimeError, match="route='band'.* needs a HIP device"):
        torbi_amd.sample_paths(obs, route='band', **args)
    with pytest.raises(RuntimeError, match='no transition matrix'):
        torbi_amd.sample_paths(obs, draws=3, uniforms=u, route='band', gpu=0)
    # a matrix that has no band viterbi.band_over can answer for (here: 4 states, and on the host) has no plan
    plan, why = sampling._band_plan(A, A, 2, 5, 4, 3, 0)
    assert plan is None and 'does not hold one value outside a band' in why
    # 'auto' and 'dense' with gpu=None stay the float64 dense rule
    auto = torbi_amd.sample_paths(obs, route='auto', **args)
    dense = torbi_amd.sample_paths(obs, **args)
    assert torch.equal(auto[0], dense[0]) and torch.equal(auto[1], dense[1])
    assert torbi_amd.sample_route(None, 2, 5, 4) == 'uniform' and torbi_amd.sample_route(A, 2, 5, 4, gpu=None) == 'dense'
    with pytest.raises(RuntimeError, match='transition must have shape'):
        torbi_amd.sample_route(A[:3], 2, 5, 4)
    with pytest.raises(RuntimeError, match='draws must be'):
        torbi_amd.sample_route(A, 2, 5, 4, draws=0)


def test_auto_takes_the_band_only_in_measured_classes():
    """`_band_pays(batch, states, reach_left, reach_right, draws)` encodes the probe's table (SAMPLING.md, "Band route"): 23
    diagonals of 1440 states at 1, 8 and 512 items with one draw, and at 512 items with 16 draws.  Nothing else is taken."""
    pays = sampling._band_pays
    for batch in (1, 8, 512):
        assert pays(batch, 1440, 11, 11, 1)
    assert pays(512, 1440, 11, 11, 16) and pays(512, 1440, 0, 0, 16) and pays(100, 360, 2, 2, 1)
    assert not pays(512, 1440, 11, 11, 17)                      # more draws than were measured
    assert not pays(8, 1440, 11, 11, 2) and not pays(511, 1440, 11, 11, 16)     # several draws at another batch size
    assert not pays(513, 1440, 11, 11, 1)                       # a larger batch
    assert not pays(512, 1440, 12, 11, 1)                       # a wider band
    assert not pays(6, 360, 11, 11, 1)                          # 23 of 360: a larger share of the row
