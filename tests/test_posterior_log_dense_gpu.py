"""The dense log-space route of the state posteriors on an MI355X (csrc/forward_backward_log.hpp, torbi_amd.forward_backward_log
and state_posteriors(route='log-dense')) against the float64 log-space reference of tests/test_posterior_log_band_gpu.py on
the same log inputs, within the bounds of tests/test_posterior_band_gpu.py::check (which prints every figure first).  The
tile rule wants 8 workgroups for each of the 256 compute units: with one state block TB = 1 below 4095 items, 2 at 4099, 4
at 8194 and 8 at 16386.
"""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, inputs, synth
from test_posterior_band_gpu import DEV, check, ragged, same, to_dev
from test_posterior_log_band_gpu import log_space

pytestmark = pytest.mark.gpu

NINF = -math.inf
TILES = {5: 1, 4099: 2, 8194: 4, 16386: 8}         # batch -> TB at (T, S) = (3, 33), every last tile partial
SHAPES = [(1, 1, 8),                               # one frame reads no matrix entry
          (3, 40, 64),                             # ragged lengths 40, 1, 2
          (17, 33, 65),                            # one state past a block
          (9, 12, 37),                             # less than a block: slices of three quads, the last of one
          (5, 30, 257),
          (2, 6, 1441)] + [(B, 3, 33) for B in TILES]     # odd S, several blocks, long slices; every TB
WIDE_RANGE = [(3, 24, 64), (3, 50, 200), (2, 40, 128)]     # dense; left-to-right with skips; permutation + log(1e-30)


@functools.lru_cache(maxsize=None)
def problem(B, T, S):
    """(observation, frames, transition, initial) of one case, read-only."""
    if (B, T, S) in WIDE_RANGE:
        g = torch.Generator().manual_seed(5)
        obs = torch.log_softmax(12 * torch.randn(B, T, S, generator=g), 2).numpy()
        init = torch.log_softmax(torch.randn(S, generator=g), 0).numpy()
        frames = np.full(B, T, dtype=np.int32)
        if S == 64:
            trans = torch.log_softmax(4 * torch.randn(S, S, generator=g), 0).numpy()
        elif S == 200:                                                # [next, prev]: next >= prev, columns normalised
            below = torch.tril(torch.ones(S, S)) > 0
            trans = torch.log_softmax(torch.randn(S, S, generator=g).masked_fill(~below, NINF), 0).numpy()
            init = np.where(np.arange(S) == 0, 0., NINF).astype(np.float32)
        else:
            trans = np.full((S, S), math.log(1e-30), dtype=np.float32)
            trans[torch.randperm(S, generator=g).numpy(), np.arange(S)] = 0.
    else:
        seed = B + T + S
        obs = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), seed)
        init = synth.scores(synth.STREAM_INITIAL, (S,), seed)
        frames = ragged(B, T, seed=S)
        trans = synth.scores(synth.STREAM_TRANSITION, (S, S), seed)
        trans = np.where(synth.scores(synth.STREAM_TRANSITION, (S, S), seed + 1) > -1.6, np.float32(NINF), trans)   # a tenth
    out = (obs, frames, trans, init)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(*case):
    return log_space(*problem(*case))


def device(obs, frames, trans, init, workspace=None):
    g, L = torbi_amd.forward_backward_log(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), workspace=workspace)
    return g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)


def all_nan(got, frames, items):
    g, L = got
    F = np.clip(frames, 1, g.shape[1])
    return all(np.isnan(L[b]) and np.isnan(g[b, :F[b]]).all() and (g[b, F[b]:] == 0).all() for b in items)


@pytest.mark.parametrize('case', SHAPES + WIDE_RANGE, ids=lambda c: 'x'.join(map(str, c)))
def test_against_float64_log_space(case):
    B, _, S = case
    if B in TILES:
        assert _lib.load().torbi_hip_forward_backward_log_tile(B, S, 0) == TILES[B]
    assert np.isfinite(reference(*case)[1]).all()
    check(device(*problem(*case)), reference(*case), problem(*case)[1])


def test_state_posteriors_takes_the_route_where_the_scaled_one_fails():
    case = WIDE_RANGE[0]
    obs, frames, trans, init = (torch.from_numpy(np.array(a)) for a in problem(*case))
    g, L = torbi_amd.state_posteriors(obs, frames, trans, init, log_probs=True, gpu=0, route='log-dense')
    prepared, _, init_d = inputs.model(trans, init, True, case[2], DEV)                # the model and the observation it ran on
    want = log_space(inputs.observation(obs, True, DEV), frames.to(DEV), prepared, init_d)
    check((g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)), want, frames.numpy())


def test_an_item_s_bits_depend_neither_on_its_tile_nor_on_the_batch():
    obs, frames, trans, init = problem(8194, 3, 33)
    whole = device(obs, frames, trans, init)                              # TB = 4
    for rows in (slice(0, 1), slice(8193, 8194)):                         # TB = 1; the partial tile's last item alone
        assert same(device(obs[rows], frames[rows], trans, init), (whole[0][rows], whole[1][rows]))


@pytest.mark.parametrize('value', [math.nan, math.inf])
def test_a_nan_or_inf_observation_stays_in_its_item(value):
    obs, frames, trans, init = problem(3, 40, 64)                         # frames 40, 1, 2
    clean = device(obs, frames, trans, init)
    bad = np.array(obs)
    bad[0, 17, 9] = value
    got = device(bad, frames, trans, init)
    assert all_nan(got, frames, [0]) and same((got[0][1:], got[1][1:]), (clean[0][1:], clean[1][1:]))


def test_an_impossible_start_is_minus_infinity_and_nan_rows():
    obs, frames, trans, _ = problem(3, 40, 64)
    g, L = device(obs, frames, trans, np.full(64, NINF, dtype=np.float32))
    assert (L == NINF).all() and all_nan((g, L * math.nan), frames, range(3))


def test_a_caller_owned_workspace_and_a_captured_graph():
    case = (17, 33, 65)
    obs, frames, trans, init = problem(*case)
    obs2 = synth.scores(synth.STREAM_OBSERVATION, case, 99)
    need = torbi_amd.forward_backward_log_workspace_bytes(*case)
    ws = torch.full((need + 3,), 0xFF, dtype=torch.uint8, device=DEV)[3:]              # stale bytes at an odd base address
    tobs, tframes, ttrans, tinit = (to_dev(a) for a in (obs, frames, trans, init))
    run = lambda o: torbi_amd.forward_backward_log(o, tframes, ttrans, tinit, workspace=ws)
    eager, eager2 = [x.clone() for x in run(tobs)], [x.clone() for x in run(to_dev(obs2))]
    fresh = torbi_amd.forward_backward_log(tobs, tframes, ttrans, tinit)
    assert ws.data_ptr() % 2 == 1 and torch.equal(eager[0], fresh[0]) and torch.equal(eager[1], fresh[1])
    assert not torch.equal(eager[0], eager2[0])
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
