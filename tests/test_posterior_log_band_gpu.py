"""The log-space band route of the state posteriors on an MI355X (csrc/forward_backward_log_band.hpp,
torbi_amd.forward_backward_log_banded and state_posteriors(arithmetic='log')) against a float64 log-space reference on the same
log inputs, within the bounds of tests/test_posterior_gpu.py::check (tests/test_posterior_band_gpu.py's copy prints every
figure first).  The tile rule at 256 compute units gives G = 1 below 512 items, G = 2 at 515 and G = 4 at 2050.
"""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, inputs, synth
from test_posterior_band_gpu import DEV, NINF, TINY, check, ragged, same, to_dev

pytestmark = pytest.mark.gpu

# B, T, S, reach_left, reach_right, background
SHAPES = [(1, 1, 8, 1, 1, NINF),                   # one frame reads no matrix entry
          (3, 40, 64, 2, 5, NINF),                 # asymmetric reaches, ragged lengths
          (3, 40, 64, 5, 2, -20.0),                # ... and a finite background
          (17, 33, 65, 0, 0, NINF),                # zero reach
          (9, 12, 37, 36, 36, -3.0),               # the band clipped to the whole matrix
          (5, 30, 1441, 12, 12, NINF),             # odd S, unaligned rows
          (2, 30, 300, 87, 87, NINF),              # 175 diagonals: several dquads and slices
          (2, 30, 300, 87, 87, TINY),              # ... log(tiny) outside
          (2, 6, 4096, 255, 256, NINF),            # W = 512, the limit
          (515, 4, 65, 2, 1, -6.0),                # G = 2 and a partial last tile
          (2050, 3, 33, 0, 3, NINF)]               # G = 4 and a partial last tile
# where the scaled recurrence fails (float32 emulation: NaN rows and L off by 18.2; gamma and L off by 1.4e-2; by 9e-4),
# and a left-to-right matrix from a one-hot start
WIDE_RANGE = [(3, 24, 64, 1, 1, NINF), (2, 40, 257, 3, 3, NINF), (2, 200, 64, 1, 1, TINY), (3, 50, 200, 1, 0, NINF)]


@functools.lru_cache(maxsize=None)
def problem(B, T, S, reach_left, reach_right, background):
    """(observation, frames, transition, initial) of one case, read-only."""
    if (B, T, S, reach_left, reach_right, background) in WIDE_RANGE:
        g = torch.Generator().manual_seed(5)
        left_to_right = reach_right == 0
        obs = torch.log_softmax((3 if left_to_right else 12) * torch.randn(B, T, S, generator=g), 2).numpy()
        init = torch.log_softmax(torch.randn(S, generator=g), 0).numpy()
        frames = np.full(B, T, dtype=np.int32)
        if left_to_right:
            trans = np.full((S, S), NINF, dtype=np.float32)
            trans[np.arange(S), np.arange(S)] = trans[np.arange(1, S), np.arange(S - 1)] = math.log(0.5)
            trans[S - 1, S - 1] = 0.                                  # the last state is absorbing
            init = np.where(np.arange(S) == 0, 0., NINF).astype(np.float32)
        else:
            trans = synth.banded_transition(S, reach_left + 1, tiny=background != NINF)
    else:
        seed = B + T + S
        obs = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), seed)
        init = synth.scores(synth.STREAM_INITIAL, (S,), seed)
        frames = ragged(B, T, seed=S)
        if S == 300:
            trans = synth.banded_transition(S, 88, tiny=background != NINF)
        else:                                                         # random band entries, none under the background
            j, i = np.arange(S)[:, None], np.arange(S)[None, :]
            inside = (i >= j - reach_left) & (i <= j + reach_right)
            entries = np.maximum(synth.scores(synth.STREAM_TRANSITION, (S, S), seed), np.float32(background))
            trans = np.where(inside, entries, np.float32(background)).astype(np.float32)
    out = (obs, frames, trans, init)
    for a in out:
        a.setflags(write=False)
    return out


def log_space(obs, frames, trans, init):
    """Forward-backward in float64 log space with plain torch ops, where the inputs are (arrays: on the host): (gamma, L),
    rows t >= F zero."""
    o, A, pi, F = (a if torch.is_tensor(a) else torch.from_numpy(np.array(a)) for a in (obs, trans, init, frames))
    o, A, pi = o.double(), A.double(), pi.double()
    B, T, S = o.shape
    F = F.long().clamp(1, T)
    la, lb = torch.empty_like(o), torch.zeros_like(o)
    la[:, 0] = pi + o[:, 0]
    for t in range(1, T):
        la[:, t] = o[:, t] + torch.logsumexp(A[None] + la[:, t - 1, None, :], 2)
    for t in range(T - 2, -1, -1):
        step = torch.logsumexp(A.T[None] + (o[:, t + 1] + lb[:, t + 1])[:, None, :], 2)
        lb[:, t] = torch.where((t < F - 1)[:, None], step, torch.zeros_like(step))
    L = torch.logsumexp(la[torch.arange(B, device=o.device), F - 1], 1)
    valid = (torch.arange(T, device=o.device)[None, :] < F[:, None])[..., None]
    return torch.where(valid, torch.exp(la + lb - L[:, None, None]), torch.zeros_like(o)).cpu().numpy(), L.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(*case):
    return log_space(*problem(*case))


def device(obs, frames, trans, init, reach_left, reach_right, background, workspace=None):
    g, L = torbi_amd.forward_backward_log_banded(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), reach_left,
                                                 reach_right, background, workspace=workspace)
    return g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)


def all_nan(got, frames, items):
    g, L = got
    F = np.clip(frames, 1, g.shape[1])
    return all(np.isnan(L[b]) and np.isnan(g[b, :F[b]]).all() and (g[b, F[b]:] == 0).all() for b in items)


@pytest.mark.parametrize('case', SHAPES + WIDE_RANGE, ids=lambda c: 'x'.join(map(str, c[:3])) + f'-{c[3]}-{c[4]}-{c[5]:.0f}')
def test_against_float64_log_space(case):
    B, S = case[0], case[2]
    if B in (515, 2050):
        assert _lib.load().torbi_hip_forward_backward_log_band_tile(B, S, case[3], case[4], 0) == {515: 2, 2050: 4}[B]
    check(device(*problem(*case), *case[3:]), reference(*case), problem(*case)[1])


def test_state_posteriors_takes_the_route_where_the_scaled_one_fails():
    case = WIDE_RANGE[0]
    obs, frames, trans, init = (torch.from_numpy(np.array(a)) for a in problem(*case))
    g, L = torbi_amd.state_posteriors(obs, frames, trans, init, log_probs=True, gpu=0, route='band', arithmetic='log')
    prepared, _, init_d = inputs.model(trans, init, True, case[2], DEV)                # the model and the observation it ran on
    want = log_space(inputs.observation(obs, True, DEV), frames.to(DEV), prepared, init_d)
    check((g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)), want, frames.numpy())
    with pytest.raises(RuntimeError, match='band route only.*gpu=None'):
        torbi_amd.state_posteriors(-torch.rand(1, 2, 320), None, -torch.rand(320, 320), log_probs=True, gpu=0,
                                   arithmetic='log')                                   # dense: no band of up to 512 entries


def test_an_item_s_bits_depend_neither_on_its_tile_nor_on_the_batch():
    case = (515, 4, 65, 2, 1, -6.0)
    obs, frames, trans, init = problem(*case)
    whole = device(obs, frames, trans, init, *case[3:])                  # G = 2
    for rows in (slice(0, 1), slice(514, 515)):                           # G = 1; the partial tile's item alone
        assert same(device(obs[rows], frames[rows], trans, init, *case[3:]), (whole[0][rows], whole[1][rows]))


@pytest.mark.parametrize('value', [math.nan, math.inf])
def test_a_nan_or_inf_observation_stays_in_its_item(value):
    case = (3, 40, 64, 2, 5, NINF)
    obs, frames, trans, init = problem(*case)                            # frames 40, 1, 2
    clean = device(obs, frames, trans, init, *case[3:])
    bad = np.array(obs)
    bad[0, 17, 9] = value
    got = device(bad, frames, trans, init, *case[3:])
    assert all_nan(got, frames, [0]) and same((got[0][1:], got[1][1:]), (clean[0][1:], clean[1][1:]))


def test_an_impossible_start_is_minus_infinity_and_nan_rows():
    case = (3, 40, 64, 2, 5, NINF)
    obs, frames, trans, init = problem(*case)
    g, L = device(obs, frames, trans, np.full(64, NINF, dtype=np.float32), *case[3:])
    assert (L == NINF).all() and all_nan((g, L * math.nan), frames, range(3))


@pytest.mark.parametrize('case,at,value', [((3, 40, 64, 2, 5, NINF), (60, 3), -1.0),      # outside the band, not `background`
                                           ((3, 40, 64, 5, 2, -20.0), (60, 3), -1.0),
                                           ((3, 40, 64, 5, 2, -20.0), (30, 28), -21.0)])   # inside it, under the background
def test_a_broken_promise_is_nan(case, at, value):
    obs, frames, trans, init = problem(*case)
    broken = np.array(trans)
    broken[at] = value
    assert all_nan(device(obs, frames, broken, init, *case[3:]), frames, range(case[0]))


def test_a_caller_owned_workspace_and_a_captured_graph():
    case = (3, 40, 64, 5, 2, -20.0)
    obs, frames, trans, init = problem(*case)
    obs2 = synth.scores(synth.STREAM_OBSERVATION, case[:3], 99)
    ws = torch.full((torbi_amd.forward_backward_log_banded_workspace_bytes(*case[:5]),), 0xFF, dtype=torch.uint8, device=DEV)
    tobs, tframes, ttrans, tinit = (to_dev(a) for a in (obs, frames, trans, init))
    run = lambda o: torbi_amd.forward_backward_log_banded(o, tframes, ttrans, tinit, *case[3:], workspace=ws)
    eager, eager2 = [x.clone() for x in run(tobs)], [x.clone() for x in run(to_dev(obs2))]
    fresh = torbi_amd.forward_backward_log_banded(tobs, tframes, ttrans, tinit, *case[3:])
    assert torch.equal(eager[0], fresh[0]) and torch.equal(eager[1], fresh[1]) and not torch.equal(eager[0], eager2[0])
    side, graph = torch.cuda.Stream(device=DEV), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            post, loglik = run(tobs)
    for want in (eager, eager, eager2):                                  # two replays on the captured inputs, one on new ones
        if want is eager2:
            tobs.copy_(to_dev(obs2))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(post, want[0]) and torch.equal(loglik, want[1])
