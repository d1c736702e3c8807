"""The band route of k-best decoding without a device: the numpy restatement of its rule (k_best_band_cases.restate: dmax,
fast path, fallback) against the host route and the brute-force enumerator, that the test inputs take both paths, and the
C-ABI and Python surface of the route."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib
import k_best_cases as kc
import k_best_band_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64
KS = [1, 2, 3, 4, 8, 32]


def host(obs, frames, trans, init, k):
    i, s = torbi_amd.decode_k_best(torch.as_tensor(obs), torch.as_tensor(frames), torch.as_tensor(trans), torch.as_tensor(init), k)
    return i.numpy(), s.numpy()


def frames_of(B, T):
    return np.array([T] + [max(1, T - 1 - b) for b in range(B - 1)], dtype=np.int32)


def check(obs, frames, trans, init, k, reach, background):
    i, s, path, equal = bc.restate(obs, frames, trans, init, k, reach[0], reach[1], background)
    kc.same((i, s), host(obs, frames, trans, init, k))
    return path, equal


# ------------------------------------------------------------------------------------------ 1: the rule is the dense result
@pytest.mark.parametrize('background', bc.BACKGROUNDS, ids=['inf', 'tiny', 'm20'])
@pytest.mark.parametrize('reach', bc.REACHES, ids=lambda r: f'{r[0]}-{r[1]}')
def test_restatement_is_the_host_route_on_continuous_scores(reach, background):
    B, T = 3, 5
    for k in KS:
        obs, trans, init = bc.model(B, T, S, 11 + k, reach, background)
        path, _ = check(obs, frames_of(B, T), trans, init, k, reach, background)
        fast, fallback = bc.shares(path)
        assert fast + fallback == int((frames_of(B, T) - 1).sum()) * S
        if background == -math.inf and reach[0] + reach[1] + 1 >= k:
            # every list is full of finite values from frame 1 on at the inner states: nothing but edges falls back
            assert fast > 0


@pytest.mark.parametrize('dead', [False, True], ids=['grid', 'grid-inf'])
@pytest.mark.parametrize('background', bc.BACKGROUNDS, ids=['inf', 'tiny', 'm20'])
@pytest.mark.parametrize('reach', bc.REACHES, ids=lambda r: f'{r[0]}-{r[1]}')
def test_restatement_is_the_host_route_on_tie_grids(reach, background, dead):
    B, T = 3, 5
    for k, levels in ((1, 3), (2, 3), (3, 3), (4, 12), (8, 3), (32, 12)):
        obs, trans, init = bc.model(B, T, S, 5 + k, reach, background, levels=levels, dead=dead)
        check(obs, frames_of(B, T), trans, init, k, reach, background)


@pytest.mark.parametrize('k', [2, 8])
def test_restatement_ragged_from_one_frame(k):
    """An item of one frame beside longer ones, on a grid with -inf entries."""
    B, T, reach = 4, 6, (5, 2)
    obs, trans, init = bc.model(B, T, S, 77, reach, -20., levels=6, dead=True)
    check(obs, np.array([1, 6, 2, 4], dtype=np.int32), trans, init, k, reach, -20.)


@pytest.mark.parametrize('background', bc.BACKGROUNDS, ids=['inf', 'tiny', 'm20'])
@pytest.mark.parametrize('states,reach', [(2, (0, 0)), (3, (1, 0)), (3, (0, 1)), (4, (1, 1)), (4, (0, 2))])
def test_restatement_against_brute_force(states, reach, background):
    """Sizes the enumerator can rank: lists that grow over several frames, more ranks than paths, ragged frames."""
    B, T = 3, 5
    frames = np.array([5, 3, 1], dtype=np.int32)
    for k in (1, 2, 3, 4, 8, 32):
        for levels, dead in ((None, False), (3, False), (3, True)):
            obs, trans, init = bc.model(B, T, states, 3 + k, reach, background, levels=levels, dead=dead)
            i, s, _, _ = bc.restate(obs, frames, trans, init, k, reach[0], reach[1], background)
            kc.same((i, s), kc.brute(obs, frames, trans, init, k))


# --------------------------------------------------------------------------------------- 2: the inputs take both paths
@pytest.mark.parametrize('reach,background,k,levels,dead', bc.BOTH, ids=bc.BOTH_IDS)
def test_tie_and_inf_inputs_take_both_paths(reach, background, k, levels, dead):
    """On the restatement: at least 64 (item, frame, state) cells on each path, and a cell whose full in-band list has a
    k-th value EQUAL to dmax -- a strict '>' sends it to the fallback, where the equal out-of-band candidate stays out."""
    obs, frames, trans, init = bc.both_problem(reach, background, levels, dead)
    path, equal = check(obs, frames, trans, init, k, reach, background)
    fast, fallback = bc.shares(path)
    print(f'reach {reach}, background {background}, k {k}: fast {fast}, fallback {fallback}, k-th == dmax {int(equal.sum())}')
    assert fast >= 64 and fallback >= 64, (fast, fallback)
    assert equal.any() and (path[equal] == bc.FALLBACK).all()


@pytest.mark.parametrize('k', [1, 2, 4])
def test_an_equal_candidate_left_of_the_band_decides_the_result(k):
    """The one place where '>=' against dmax would change a bit: a full in-band list whose k-th value equals an out-of-band
    candidate of a LOWER prev-state.  The rule (and the host route) point at that prev-state; the '>=' variant of the
    restatement does not, and the difference reaches the result, so a device test on this input tells the two apart."""
    obs, frames, trans, init, reach, background = bc.tie_left_of_band(k)
    path, equal = check(obs, frames, trans, init, k, reach, background)
    assert equal[:, 0, 40].all() and (path[:, 0, 40] == bc.FALLBACK).all()
    right = bc.restate(obs, frames, trans, init, k, reach[0], reach[1], background)
    wrong = bc.restate(obs, frames, trans, init, k, reach[0], reach[1], background, strict=False)
    assert (right[0][:, :, 1] == 40).all() and (right[0][:, :, 0] == np.arange(k)).all()        # out of band, left, first
    assert (wrong[0][:, :, 1] == 40).all() and (wrong[0][:, :, 0] == 38 + np.arange(k)).all()   # what '>=' would give


# --------------------------------------------------------------------------------------------------------- 3: surface
BAND_SYMBOLS = ['torbi_hip_k_best_band_covers', 'torbi_hip_k_best_band_workspace_bytes', 'torbi_hip_k_best_band']


def test_symbols_are_declared_and_exported_within_abi_17():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    for name in BAND_SYMBOLS:
        assert re.search(r'\b(?:int|size_t) ' + name + r'\s*\(', header), name
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert re.search(r'#define TORBI_HIP_ABI_VERSION 17\b', header)
    for name in ('decode_k_best_banded', 'decode_k_best_banded_workspace_bytes', 'k_best_route'):
        assert name in torbi_amd.__all__ and callable(getattr(torbi_amd, name))


def test_covers_answers_without_a_device():
    covers = _lib.load().torbi_hip_k_best_band_covers
    f = ctypes.c_float
    for bg in bc.BACKGROUNDS:
        for k in range(1, 9):
            assert covers(1, 1, 1440, k, 87, 87, f(bg), 0) == 1 and covers(512, 500, 1440, k, 87, 87, f(bg), 0) == 1
        assert covers(3, 5, 64, 32, 0, 0, f(bg), 0) == 1 and covers(1, 2, 3072, 1, 254, 254, f(bg), 0) == 1
    # the stated rule: the two list buffers of one item within 159 KB of LDS
    for states, k, left, right in [(1440, 12, 87, 87), (1440, 13, 87, 87), (1440, 13, 11, 11), (1440, 14, 11, 11),
                                   (64, 32, 31, 31), (256, 32, 31, 31), (640, 32, 0, 0), (3072, 6, 2, 2), (3072, 7, 2, 2)]:
        assert covers(2, 3, states, k, left, right, f(-math.inf), 0) == int(bc.covered(states, k, left, right)), (states, k)
    assert bc.covered(1440, 12, 87, 87) and not bc.covered(1440, 13, 87, 87)
    assert covers(1, 2, 1440, 4, 87, 87, f(math.nan), 0) == 0 and covers(1, 2, 1440, 4, 87, 87, f(math.inf), 0) == 0
    for states in (1438, 1441, 66, 60, 3076):
        assert covers(1, 2, states, 4, 2, 2, f(-math.inf), 0) == 0, states
    assert covers(1, 2, 1440, 1, 254, 255, f(0.), 0) == 0 and covers(1, 2, 1440, 4, -1, 2, f(0.), 0) == 0
    assert covers(0, 2, 1440, 4, 2, 2, f(0.), 0) == 0 and covers(1, 0, 1440, 4, 2, 2, f(0.), 0) == 0
    assert covers(1, 2, 1440, 0, 2, 2, f(0.), 0) == 0 and covers(1, 2, 1440, 33, 2, 2, f(0.), 0) == 0


def test_workspace_bytes_follow_the_layout():
    lib = _lib.load()

    def pieces(B, T, states, k, W):
        up = lambda x: -(-x // 256) * 256
        return (up(8 * B * k * states) + up(4 * B * (T - 1) * k * states) + up(4 * W * states) + up(12 * B * k) + up(4 * B)
                + up(4 * (B + 1)) + 256 + 256)

    for B, T, states, k, left, right in [(3, 5, 64, 4, 2, 2), (512, 500, 1440, 4, 87, 87), (7, 1, 256, 8, 0, 3)]:
        need = lib.torbi_hip_k_best_band_workspace_bytes(B, T, states, k, left, right)
        assert need == pieces(B, T, states, k, left + right + 1)
        assert torbi_amd.decode_k_best_banded_workspace_bytes(B, T, states, k, left, right) == need
    # the diagonals (rounded up to a 256-byte piece) stand where the transposed matrix stood; one more piece for the verdict
    assert (lib.torbi_hip_k_best_workspace_bytes(512, 500, 1440, 4) - lib.torbi_hip_k_best_band_workspace_bytes(512, 500, 1440, 4, 87, 87)
            == 4 * 1440 * 1440 - (4 * 175 * 1440 + 128) - 256)
    assert lib.torbi_hip_k_best_band_workspace_bytes(0, 5, 64, 4, 2, 2) == 256
    assert lib.torbi_hip_k_best_band_workspace_bytes(3, 5, 64, 4, -1, 2) == 256


def test_band_entry_answers_bad_arguments_before_any_device_work():
    lib = _lib.load()
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -5
    p = ctypes.c_void_p(16)                  # never dereferenced: every call below fails its argument check first
    st = ctypes.c_void_p(0)
    B, T, states, k = 3, 5, 64, 4
    need = lib.torbi_hip_k_best_band_workspace_bytes(B, T, states, k, 2, 2)

    def call(obs=p, frames=p, trans=p, init=p, left=2, right=2, bg=-math.inf, indices=p, scores=p, ws=p, nbytes=need, B=B, T=T,
             S=states, k=k):
        return lib.torbi_hip_k_best_band(obs, frames, trans, init, left, right, ctypes.c_float(bg), indices, scores, ws, nbytes,
                                         B, T, S, k, 0, st)

    assert call(nbytes=need - 1) == EWORKSPACE
    assert call(left=-1) == EINVAL and call(right=-1) == EINVAL
    assert call(T=0) == EINVAL and call(S=0) == EINVAL and call(B=-1) == EINVAL and call(k=0) == EINVAL and call(k=33) == EINVAL
    for name in ('obs', 'frames', 'trans', 'init', 'indices', 'scores', 'ws'):
        assert call(**{name: None}) == EINVAL, name
    assert call(S=66) == EUNSUPPORTED and call(S=60) == EUNSUPPORTED and call(S=3076) == EUNSUPPORTED
    assert call(bg=math.nan) == EUNSUPPORTED and call(bg=math.inf) == EUNSUPPORTED
    assert call(left=254, right=255) == EUNSUPPORTED
    assert call(S=1440, k=13, left=87, right=87, nbytes=1 << 40) == EUNSUPPORTED     # the lists of one item beyond the LDS
    assert call(obs=None, frames=None, trans=None, init=None, indices=None, scores=None, ws=None, nbytes=0, B=0) == 0


def test_route_is_an_argument_and_the_host_ignores_it():
    assert inspect.signature(torbi_amd.best_paths).parameters['route'].default == 'auto'
    assert inspect.signature(torbi_amd.decode_k_best).parameters['route'].default == 'auto'
    assert torbi_amd.k_best_route(None, 2, 5, 64, 4, gpu=None) == 'host'
    assert torbi_amd.k_best_route(torch.zeros((64, 64)), 2, 5, 64, 4, gpu=None, log_probs=True) == 'host'
    B, T, k, reach = 2, 4, 3, (2, 2)
    obs, trans, init = bc.model(B, T, S, 3, reach, -math.inf)
    frames = frames_of(B, T)
    want = bc.restate(kc.clamp(obs), frames, trans, init, k, 2, 2, -math.inf)[:2]
    for route in ('auto', 'dense', 'band'):
        got = torbi_amd.best_paths(torch.as_tensor(obs), k, torch.as_tensor(frames), torch.as_tensor(trans), torch.as_tensor(init),
                                   log_probs=True, gpu=None, route=route)
        kc.same((got[0].numpy(), got[1].numpy()), want)
        got = torbi_amd.decode_k_best(torch.as_tensor(kc.clamp(obs)), torch.as_tensor(frames), torch.as_tensor(trans),
                                      torch.as_tensor(init), k, route=route)
        kc.same((got[0].numpy(), got[1].numpy()), want)
    with pytest.raises(ValueError):
        torbi_amd.best_paths(torch.as_tensor(obs), k, gpu=None, route='bogus')
    with pytest.raises(ValueError):
        torbi_amd.decode_k_best(torch.as_tensor(obs), None, torch.as_tensor(trans), torch.as_tensor(init), k, route='bogus')
    with pytest.raises(RuntimeError, match='HIP device'):
        torbi_amd.decode_k_best_banded(torch.as_tensor(obs), None, torch.as_tensor(trans), torch.as_tensor(init), k, 2, 2)


def test_instance_rule():
    """The (KMAX, G) a shape runs, by the rule the header states: what the device tests choose their batch sizes from."""
    assert bc.instance(512, 1440, 4, 87, 87) == (4, 2) and bc.instance(512, 1440, 8, 87, 87) == (8, 1)
    assert bc.instance(1023, 64, 1, 2, 2) == (1, 4) and bc.instance(511, 64, 1, 2, 2) == (1, 2) and bc.instance(510, 64, 1, 2, 2) == (1, 1)
    assert bc.instance(1023, 64, 8, 2, 2) == (8, 2) and bc.instance(1023, 64, 9, 2, 2) == (16, 1)
