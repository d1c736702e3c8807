"""The wide band route of the state posteriors on an MI355X (csrc/forward_backward_wide_band.hpp,
torbi_amd.forward_backward_wide_banded and the routing of torbi_amd.state_posteriors) against the float64 host route on the
same log inputs, within the bounds of tests/test_posterior_gpu.py::check.  Helpers are tests/test_posterior_band_gpu.py's.
"""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, inputs, synth
from test_posterior_band_gpu import DEV, NINF, TINY, band_matrix, check, host, peaked, ragged, same, to_dev

pytestmark = pytest.mark.gpu

# B, T, S, reach_left, reach_right, background
CASES = [(1, 1, 8, 7, 7, NINF),                    # one frame reads no matrix entry; the band clipped to the matrix
         (3, 12, 72, 40, 30, NINF),                # just past 64 entries, asymmetric, S no multiple of 64
         (3, 12, 72, 30, 40, -20.0),               # a finite background: both rank-one terms
         (2, 9, 131, 130, 130, -3.0),              # the band is the whole matrix; odd S, a ragged last quad of states
         (5, 8, 1440, 87, 87, NINF),               # the pitch matrix of 175 diagonals, peaked rows
         (5, 8, 1440, 87, 87, TINY),               # ... log(tiny) outside
         (2, 4, 4096, 255, 256, NINF),             # the widest band, the most states
         (3, 3, 68, 40, 33, NINF),                 # G = 1
         (515, 3, 68, 40, 33, NINF),               # G = 2 and a partial last tile
         (1030, 3, 68, 40, 33, NINF)]              # G = 4 and a partial last tile
TILES = {3: 1, 515: 2, 1030: 4}                    # the G rule at 256 compute units (POSTERIOR.md, "Wide band route")


@functools.lru_cache(maxsize=None)
def problem(B, T, S, reach_left, reach_right, background):
    """(observation, frames, transition, initial) of one case, read-only: the pitch matrix with peaked rows at 1440 states,
    else random band entries (not Toeplitz) and random scores."""
    if S == 1440:
        obs = peaked(B, T, S, 12, seed=1)
        trans = synth.banded_transition(S, 87.2, tiny=background != NINF)
        init = np.log(np.full(S, 1. / S, dtype=np.float32))
    else:
        seed = B + T + S
        obs = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), seed)
        init = synth.scores(synth.STREAM_INITIAL, (S,), seed)
        trans = band_matrix(S, reach_left, reach_right, background, seed)
    out = (obs, ragged(B, T, seed=S), trans, init)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(*case):
    return host(*problem(*case))


def wide(obs, frames, trans, init, reach_left, reach_right, background, workspace=None):
    """forward_backward_wide_banded on the device, the observation through the epsilon round trip as the reference sends it."""
    o = inputs.observation(torch.from_numpy(np.array(obs)), True, DEV)
    g, L = torbi_amd.forward_backward_wide_banded(o, to_dev(frames), to_dev(trans), to_dev(init), reach_left, reach_right,
                                                  background, workspace=workspace)
    return g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c[:3])) + f'-{c[3]}-{c[4]}-{c[5]:.0f}')
def test_against_float64(case):
    B, S = case[0], case[2]
    if B in TILES and S == 68:
        assert _lib.load().torbi_hip_forward_backward_wide_band_tile(B, S, case[3], case[4], 0) == TILES[B]
    check(wide(*problem(*case), *case[3:]), reference(*case), problem(*case)[1])


def test_a_nan_inside_the_band_reaches_every_item_that_takes_a_step():
    case = (3, 12, 72, 40, 30, NINF)
    obs, frames, trans, init = problem(*case)
    bad = np.array(trans)
    bad[20, 50] = np.nan                                                  # next 20, prev 50: inside reach_right = 30
    g, L = wide(obs, frames, bad, init, *case[3:])
    F = np.clip(frames, 1, case[1])
    print('frames', F, 'L', L)
    assert np.array_equal(np.isnan(L), F >= 2)
    for b in range(case[0]):
        assert np.isnan(g[b, :F[b]]).all() == (F[b] >= 2) and (g[b, F[b]:] == 0).all()


@pytest.mark.parametrize('background', [NINF, -20.0])
def test_a_broken_promise_is_nan(background):
    case = (3, 12, 72, 40, 30, background)
    obs, frames, trans, init = problem(*case)
    stray = np.array(trans)
    stray[60, 3] = -1.0                                                   # outside the stated band, not `background`
    g, L = wide(obs, frames, stray, init, *case[3:])
    F = np.clip(frames, 1, case[1])
    assert np.isnan(L).all() and all(np.isnan(g[b, :F[b]]).all() and (g[b, F[b]:] == 0).all() for b in range(case[0]))


def test_an_item_s_bits_depend_neither_on_its_tile_nor_on_the_batch():
    case = CASES[-1]
    obs, frames, trans, init = problem(*case)
    whole = wide(obs, frames, trans, init, *case[3:])                    # G = 4
    for rows in (slice(0, 1), slice(1028, 1030), slice(0, 515)):           # G = 1; G = 1 from the partial tile; G = 2
        part = wide(obs[rows], frames[rows], trans, init, *case[3:])
        assert same(part, (whole[0][rows], whole[1][rows]))


def test_a_caller_owned_workspace_of_exactly_the_queried_bytes():
    case = (3, 12, 72, 30, 40, -20.0)
    need = torbi_amd.forward_backward_wide_banded_workspace_bytes(*case[:5])
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    assert same(wide(*problem(*case), *case[3:], workspace=ws), wide(*problem(*case), *case[3:]))


@pytest.mark.parametrize('case,entry', [((3, 12, 72, 40, 30, NINF), 'forward_backward_wide_banded'),
                                        ((3, 12, 72, 30, 33, -20.0), 'forward_backward_banded')])
def test_route_band_of_state_posteriors(case, entry):
    """`route='band'`: the wide route for a band only it covers, the narrow route bit for bit for a 64-entry band."""
    obs, frames, trans, init = (torch.from_numpy(np.array(a)) for a in problem(*case))
    got = torbi_amd.state_posteriors(obs, frames, trans, init, log_probs=True, gpu=0, route='band')
    prepared, _, init_d = inputs.model(trans, init, True, case[2], DEV)
    want = getattr(torbi_amd, entry)(inputs.observation(obs, True, DEV), frames.to(DEV), prepared, init_d, *case[3:])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.isnan(got[1]).any()
