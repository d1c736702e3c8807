"""The band route of the state posteriors on an MI355X (csrc/forward_backward_band.hpp, torbi_amd.forward_backward_banded and
the routing of torbi_amd.state_posteriors) against the float64 host route on the same log inputs.

Tolerances are those of tests/test_posterior_gpu.py::check.  Every workgroup owns G whole items, G = 8 halved while the
LDS rows do not fit and while there are fewer workgroups than compute units: batches below 512 items run G = 1, so the
shapes with 515 to 4100 items are here for G = 2, 4 and 8 and their partial last tiles.
"""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import inputs, synth

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
TINY = float(np.log(np.finfo(np.float32).tiny))           # what synth.banded_transition(tiny=True) holds outside its band
NINF = -math.inf


def check(got, want, frames):
    """tests/test_posterior_gpu.py::check, printing every figure before it asserts (share of the bound in brackets)."""
    g, L = got
    rg, rL = want
    T = g.shape[1]
    F = np.clip(np.asarray(frames), 1, T)
    valid = np.arange(T)[None, :] < F[:, None]
    gamma_err = np.abs(g - rg).max()
    sum_err = np.abs(g.sum(-1) - 1)[valid].max()
    err = np.abs(L - rL)
    bound = 1e-6 * np.abs(rL) + 4e-6 * F
    print(f'shape {g.shape}: gamma {gamma_err:.2e} ({gamma_err / 1e-4:.4f}) row-sum {sum_err:.2e} ({sum_err / 1e-4:.4f}) '
          f'L {err.max():.2e} ({(err / bound).max():.4f})')
    assert gamma_err <= 1e-4, gamma_err
    assert sum_err <= 1e-4
    assert (g[~valid] == 0).all()
    assert np.all(err <= bound), (err, rL)


def ragged(B, T, seed):
    """Ragged lengths with frames[0] = T; 1, 2 and out-of-range values (clamped to [1, T]) where the batch has room."""
    frames = synth.lengths(B, -3, T + 5, seed=seed).astype(np.int32)
    for b, f in enumerate((T, 1, 2, T + 9, -2)):
        if b < B:
            frames[b] = f
    return frames


def peaked(B, T, S, half_width, seed):
    """Posteriorgram rows peaked around a pitch track that moves inside the band (log of a normalised row)."""
    rng = np.random.default_rng(seed)
    x = np.arange(S)
    obs = np.empty((B, T, S), dtype=np.float32)
    for b in range(B):
        c = rng.integers(S // 4, 3 * S // 4)
        for t in range(T):
            c = int(np.clip(c + rng.integers(-half_width + 1, half_width), 0, S - 1))
            row = np.exp(-0.5 * ((x - c) / 3.) ** 2) + 1e-3 * rng.random(S)
            obs[b, t] = np.log(row / row.sum())
    return obs


def band_matrix(S, reach_left, reach_right, background, seed):
    """Random band entries (not Toeplitz), `background` everywhere else; [next j, prev i] with j - left <= i <= j + right."""
    trans = synth.scores(synth.STREAM_TRANSITION, (S, S), seed)
    j, i = np.arange(S)[:, None], np.arange(S)[None, :]
    inside = (i >= j - reach_left) & (i <= j + reach_right)
    return np.where(inside, trans, np.float32(background)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(B, T, S, reach_left, reach_right, background):
    """(observation, frames, transition, initial) of one case, read-only.  The 1440-state cases are the pitch matrices
    with peaked rows, the others random."""
    if S == 1440:
        obs = peaked(B, T, S, 12, seed=1)
        trans = synth.banded_transition(S, 12, tiny=background != NINF)
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
    """state_posteriors(..., log_probs=True, gpu=None) on the log inputs of `problem(*case)`, computed once."""
    return host(*problem(*case))


def host(obs, frames, trans, init):
    g, L = torbi_amd.state_posteriors(torch.from_numpy(np.array(obs)), torch.from_numpy(np.array(frames)),
                                      torch.from_numpy(np.array(trans)), torch.from_numpy(np.array(init)), log_probs=True,
                                      gpu=None)
    return g.numpy().astype(np.float64), L.numpy().astype(np.float64)


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def banded(obs, frames, trans, init, reach_left, reach_right, background, clamp=True, workspace=None):
    """forward_backward_banded on the device.  clamp: the observation goes through the epsilon round trip first, as
    state_posteriors (the reference) sends it; without, the operator sees the values as they are (-inf stays -inf)."""
    o = inputs.observation(torch.from_numpy(np.array(obs)), True, DEV) if clamp else to_dev(obs)
    g, L = torbi_amd.forward_backward_banded(o, to_dev(frames), to_dev(trans), to_dev(init), reach_left, reach_right,
                                             background, workspace=workspace)
    assert g.device == DEV and g.dtype == torch.float32 and L.dtype == torch.float32
    return g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


CASES = [(1, 1, 8, 1, 1, NINF),                    # T = 1
         (3, 40, 64, 2, 5, NINF),                  # asymmetric reach: a swap of next and prev
         (3, 40, 64, 5, 2, -20.0),                 # ... the reaches swapped, a finite background
         (17, 33, 65, 0, 0, NINF),                 # diagonal only
         (9, 12, 37, 36, 36, -3.0),                # a band wider than the matrix, clipped on both edges
         (5, 30, 1441, 12, 12, NINF),              # odd S, unaligned rows
         (8, 60, 1440, 11, 11, NINF),              # the pitch matrix, -inf outside
         (8, 60, 1440, 11, 11, TINY),              # ... log(tiny) outside
         (4, 10, 4096, 31, 32, NINF),              # the largest S and W
         (70, 6, 257, 3, 0, NINF),                 # more items than one tile would hold
         (515, 4, 65, 2, 1, -6.0),                 # G = 2, partial last tile
         (1030, 3, 37, 1, 2, NINF),                # G = 4
         (2050, 3, 33, 0, 3, -9.0),                # G = 8
         (4100, 3, 360, 4, 4, NINF)]               # G = 8, two tiles per compute unit, 360 states


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_shapes_against_float64(case):
    obs, frames, trans, init = problem(*case)
    check(banded(obs, frames, trans, init, *case[3:]), reference(*case), frames)


def test_zero_probability_item():
    B, T, S = 4, 9, 64
    obs, _, trans, init = problem(3, 40, 64, 2, 2, NINF)
    obs = np.array(obs[:, :T])
    obs = np.concatenate([obs, obs[:1]])
    frames = np.array([T, 5, T, T], dtype=np.int32)
    clean = banded(obs, frames, trans, init, 2, 2, NINF, clamp=False)
    obs[2] = -np.inf
    obs[2, 0, 0] = -1.0
    obs[2, 1, 63] = -1.0                            # state 63 cannot follow state 0 inside the band
    g, L = banded(obs, frames, trans, init, 2, 2, NINF, clamp=False)
    assert L[2] == -np.inf and np.isnan(g[2]).all()
    for b in (0, 1, 3):
        assert np.array_equal(g[b], clean[0][b]) and L[b] == clean[1][b]
    assert np.isfinite(L[[0, 1, 3]]).all() and (g[1, 5:] == 0).all()


def test_nonfinite_inputs():
    B, T, S = 6, 20, 64
    obs, _, trans, init = problem(3, 40, 64, 2, 5, NINF)
    obs = np.concatenate([obs[:, :T], obs[:, T:]])
    frames = np.array([20, 20, 20, 20, 1, 9], dtype=np.int32)
    valid = np.arange(T)[None, :] < frames[:, None]
    clean = banded(obs, frames, trans, init, 2, 5, NINF)
    assert np.isfinite(clean[1]).all() and np.isfinite(clean[0]).all()
    bad = obs.copy()
    bad[1, 7, 5] = np.nan
    bad[2, 19, 63] = np.inf
    bad[4, 1, 0] = np.nan                           # beyond the item's frames
    bad[5, 12, 3] = np.inf                          # ... likewise
    g, L = banded(bad, frames, trans, init, 2, 5, NINF)
    for b in (1, 2):
        assert np.isnan(L[b]) and np.isnan(g[b]).all()
    for b in (0, 3, 4, 5):
        assert np.array_equal(g[b], clean[0][b]) and L[b] == clean[1][b]
    init2 = init.copy()
    init2[40] = np.nan
    g, L = banded(obs, frames, trans, init2, 2, 5, NINF)
    assert np.isnan(L).all() and np.isnan(g[valid]).all() and (g[~valid] == 0).all()
    for value in (np.nan, np.inf):
        t2 = trans.copy()
        t2[30, 33] = value                          # inside the band: i = j + 3
        g, L = banded(obs, frames, t2, init, 2, 5, NINF)
        steps = frames >= 2
        assert np.isnan(L[steps]).all() and np.isnan(g[steps][valid[steps]]).all()
        assert np.array_equal(g[4], clean[0][4]) and L[4] == clean[1][4]        # one frame: the matrix is not read
        assert (g[~valid] == 0).all()


def test_broken_promise_is_loud():
    case = (3, 40, 64, 2, 2, NINF)
    obs, frames, trans, init = problem(*case)
    trans = trans.copy()
    trans[20, 23] = -1.5                            # just outside the stated band: i = j + reach_right + 1
    g, L = banded(obs, frames, trans, init, 2, 2, NINF)
    F = np.clip(frames, 1, 40)
    valid = np.arange(40)[None, :] < F[:, None]
    assert np.isnan(L).all() and np.isnan(g[valid]).all() and (g[~valid] == 0).all()
    check(banded(obs, frames, trans, init, 2, 3, NINF), host(obs, frames, trans, init), frames)


def test_bits_do_not_depend_on_the_call_the_neighbours_or_the_tile():
    B, T, S = 40, 12, 360
    obs = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), 31)
    init = synth.scores(synth.STREAM_INITIAL, (S,), 31)
    trans = band_matrix(S, 4, 4, -30.0, 31)
    frames = ragged(B, T, seed=5)
    a = banded(obs, frames, trans, init, 4, 4, -30.0)
    assert same(a, banded(obs, frames, trans, init, 4, 4, -30.0))
    other = obs.copy()
    other[1:] = synth.scores(synth.STREAM_OBSERVATION, (B - 1, T, S), 32)
    b = banded(other, frames, trans, init, 4, 4, -30.0)
    assert np.array_equal(a[0][0], b[0][0]) and a[1][0] == b[1][0]
    one = banded(obs[:1], frames[:1], trans, init, 4, 4, -30.0)
    assert np.array_equal(a[0][0], one[0][0]) and a[1][0] == one[1][0]
    # ... and in tiles of 8 items (4100 items, the last tile partial): items 0 and 4099 against batches of one
    many = np.ascontiguousarray(np.broadcast_to(obs[:20, :3], (205, 20, 3, S)).reshape(4100, 3, S))
    lengths = ragged(4100, 3, seed=6)
    big = banded(many, lengths, trans, init, 4, 4, -30.0)
    for b in (0, 4099):
        one = banded(many[b:b + 1], lengths[b:b + 1], trans, init, 4, 4, -30.0)
        assert np.array_equal(big[0][b], one[0][0]) and big[1][b] == one[1][0]


@pytest.mark.parametrize('tiny', [False, True])
def test_routing(tiny):
    B, T, S = 8, 60, 1440
    case = (B, T, S, 11, 11, TINY if tiny else NINF)
    obs, frames, trans, init = (torch.from_numpy(np.array(x)) for x in problem(*case))
    assert torbi_amd.posterior_route(trans, B, T, S, gpu=0, log_probs=True) == 'band'
    assert torbi_amd.posterior_route(None, B, T, S, gpu=0) == 'uniform'
    dense_matrix = torch.from_numpy(synth.problem(1, 1, S, seed=3)[1])
    assert torbi_amd.posterior_route(dense_matrix, B, T, S, gpu=0, log_probs=True) == 'dense'
    prepared, _, init_d = inputs.model(trans, init, True, S, DEV)
    obs_d = inputs.observation(obs, True, DEV)
    auto = torbi_amd.state_posteriors(obs, frames, trans, init, log_probs=True, gpu=0)
    band = torbi_amd.forward_backward_banded(obs_d, frames, prepared, init_d, 11, 11, case[5])
    assert torch.equal(auto[0], band[0]) and torch.equal(auto[1], band[1])
    named = torbi_amd.state_posteriors(obs, frames, trans, init, log_probs=True, gpu=0, route='band')
    assert torch.equal(auto[0], named[0]) and torch.equal(auto[1], named[1])
    dense = torbi_amd.state_posteriors(obs, frames, trans, init, log_probs=True, gpu=0, route='dense')
    plain = torbi_amd.forward_backward(obs_d, frames, prepared, init_d)
    assert torch.equal(dense[0], plain[0]) and torch.equal(dense[1], plain[1])
    with pytest.raises(RuntimeError, match='band'):
        torbi_amd.state_posteriors(obs, frames, dense_matrix, init, log_probs=True, gpu=0, route='band')
    # both device routes against float64, and against each other
    want = reference(*case)
    got_band = tuple(x.cpu().numpy().astype(np.float64) for x in auto)
    got_dense = tuple(x.cpu().numpy().astype(np.float64) for x in dense)
    check(got_band, want, frames.numpy())
    check(got_dense, want, frames.numpy())
    gap = np.abs(got_band[0] - got_dense[0]).max()
    print(f'band against dense: max |gamma_band - gamma_dense| = {gap:.2e}')
    assert gap <= 2e-4


def test_graph_capture_replays_on_new_observations():
    B, T, S = 20, 25, 400
    obs = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), 13)
    obs2 = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), 14)
    init = synth.scores(synth.STREAM_INITIAL, (S,), 13)
    trans = band_matrix(S, 6, 3, -40.0, 13)
    frames = np.clip(synth.lengths(B, 1, T, seed=5), 1, T).astype(np.int32)
    tobs, tframes, ttrans, tinit = (torch.as_tensor(np.ascontiguousarray(x)).to(DEV) for x in (obs, frames, trans, init))
    ws = torch.empty(torbi_amd.forward_backward_banded_workspace_bytes(B, T, S, 6, 3), dtype=torch.uint8, device=DEV)
    run = lambda o: torbi_amd.forward_backward_banded(o, tframes, ttrans, tinit, 6, 3, -40.0, workspace=ws)
    eager = [x.clone() for x in run(tobs)]
    eager2 = [x.clone() for x in run(torch.as_tensor(obs2).to(DEV))]
    assert not torch.equal(eager[0], eager2[0])
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            post, loglik = run(tobs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(post, eager[0]) and torch.equal(loglik, eager[1])
    tobs.copy_(torch.as_tensor(obs2))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(post, eager2[0]) and torch.equal(loglik, eager2[1])
    check((eager2[0].cpu().numpy().astype(np.float64), eager2[1].cpu().numpy().astype(np.float64)),
          host(obs2, frames, trans, init), frames)


def test_an_uncovered_band_raises():
    obs, frames, trans, init = (to_dev(x) for x in problem(3, 40, 64, 2, 5, NINF))
    wide = torch.zeros((3, 4, 130), device=DEV)
    with pytest.raises(RuntimeError, match='does not cover'):
        torbi_amd.forward_backward_banded(wide, None, torch.zeros((130, 130), device=DEV), torch.zeros(130, device=DEV),
                                          32, 32)
    with pytest.raises(RuntimeError, match='does not cover'):
        torbi_amd.forward_backward_banded(obs, frames, trans, init, 2, 5, background=math.nan)
    with pytest.raises(RuntimeError, match='>= 0'):
        torbi_amd.forward_backward_banded(obs, frames, trans, init, -1, 5)
