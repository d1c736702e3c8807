"""torbi_amd.state_posteriors / forward_backward on an MI355X (csrc/forward_backward.hpp) against the float64 host route,
which tests/test_posterior_cpu.py checks against log-space and brute-force references."""
import math

import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def host(obs, frames, trans, init):
    """The float64 route on the same (log) inputs."""
    t = None if trans is None else torch.as_tensor(trans)
    g, L = torbi_amd.state_posteriors(torch.as_tensor(obs), torch.as_tensor(frames), t, torch.as_tensor(init),
                                      log_probs=True, gpu=None)
    return g.numpy().astype(np.float64), L.numpy().astype(np.float64)


def device(obs, frames, trans, init):
    t = None if trans is None else torch.as_tensor(trans).to(DEV)
    g, L = torbi_amd.state_posteriors(torch.as_tensor(obs).to(DEV), torch.as_tensor(frames).to(DEV), t,
                                      torch.as_tensor(init).to(DEV), log_probs=True, gpu=0)
    assert g.device == DEV and g.dtype == torch.float32 and L.dtype == torch.float32
    return g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)


def check(got, want, frames):
    g, L = got
    rg, rL = want
    T = g.shape[1]
    F = np.clip(np.asarray(frames), 1, T)
    assert np.abs(g - rg).max() <= 1e-4, np.abs(g - rg).max()
    valid = np.arange(T)[None, :] < F[:, None]
    assert np.abs(g.sum(-1) - 1)[valid].max() <= 1e-4
    assert (g[~valid] == 0).all()
    err = np.abs(L - rL)
    assert np.all(err <= 1e-6 * np.abs(rL) + 4e-6 * F), (err, rL)


@pytest.mark.parametrize('B,T,S', [(1, 1, 3), (1, 500, 1440), (3, 50, 200), (17, 64, 65), (64, 100, 256), (512, 40, 1440),
                                   (4, 20, 4096), (5, 30, 1441), (9, 12, 37), (520, 8, 1441), (700, 6, 999),
                                   (2, 4, 5), (3, 5, 8), (4, 3, 31)])       # few items, few states: the direct step with KS = 1 (< 16), 2
def test_dense_shapes_against_float64(B, T, S):
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S)
    frames = np.clip(synth.lengths(B, 1, T, seed=S), 1, T).astype(np.int32)
    frames[0] = T
    check(device(obs, frames, trans, init), host(obs, frames, trans, init), frames)


def _peaked(B, T, S, half_width, seed):
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


@pytest.mark.parametrize('tiny', [False, True])
def test_peaked_rows_with_the_pitch_band(tiny):
    B, T, S = 8, 120, 1440
    obs = _peaked(B, T, S, 12, seed=1)
    trans = synth.banded_transition(S, 12, tiny=tiny)
    init = np.log(np.full(S, 1. / S, dtype=np.float32))
    frames = np.array([120, 77, 1, 2, 120, 64, 119, 30], dtype=np.int32)
    check(device(obs, frames, trans, init), host(obs, frames, trans, init), frames)


def test_ragged_lengths():
    B, T, S = 40, 60, 360
    obs, trans, init = synth.problem(B, T, S, seed=8)
    frames = synth.lengths(B, -5, T + 7, seed=2).astype(np.int32)          # out-of-range values are clamped
    check(device(obs, frames, trans, init), host(obs, frames, trans, init), frames)


@pytest.mark.parametrize('on_device', [True, False])
def test_uniform_route_on_probabilities(on_device):
    B, T, S = 33, 70, 1440
    rng = np.random.default_rng(4)
    p = rng.random((B, T, S)).astype(np.float32) ** 4
    p /= p.sum(-1, keepdims=True)
    frames = np.clip(synth.lengths(B, 1, T, seed=4), 1, T).astype(np.int32)
    src = torch.from_numpy(p)
    g, L = torbi_amd.state_posteriors(src.to(DEV) if on_device else src, torch.from_numpy(frames), gpu=0)
    rg, rL = torbi_amd.state_posteriors(src, torch.from_numpy(frames), gpu=None)
    check((g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)),
          (rg.numpy().astype(np.float64), rL.numpy().astype(np.float64)), frames)
    # and the closed form equals the dense route on the materialised matrix
    obs = torch.log(src)
    u = np.full((S, S), np.float32(math.log(1. / S)))
    init = np.full(S, np.float32(math.log(1. / S + np.finfo(np.float32).tiny)))
    dense = device(obs.numpy(), frames, u, init)
    check((g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)), dense, frames)


@pytest.mark.parametrize('uniform', [False, True])
def test_nonfinite_rules_leave_other_items_unchanged(uniform):
    B, T, S = 6, 20, 300
    obs, trans, init = synth.problem(B, T, S, seed=6)
    trans = None if uniform else trans
    frames = np.array([20, 20, 20, 20, 20, 9], dtype=np.int32)
    clean = device(obs, frames, trans, init)
    bad = obs.copy()
    bad[1, 7, 5] = np.nan
    bad[2, 3, 200] = np.inf
    bad[3, :, :] = -np.inf                      # (log(tiny) after the epsilon round trip: an ordinary small row)
    bad[5, 12, 0] = np.nan                      # beyond the item's frames
    g, L = device(bad, frames, trans, init)
    assert np.isnan(L[1]) and np.isnan(g[1, :20]).all()
    assert np.isnan(L[2]) and np.isnan(g[2, :20]).all()
    assert np.isfinite(L[3]) and np.isfinite(g[3]).all()
    for b in (0, 4, 5):
        assert np.array_equal(g[b], clean[0][b]) and L[b] == clean[1][b]
    # zero total probability: L = -inf, NaN rows; NaN / +inf in the matrix reaches every item that takes a step
    g, L = device(obs, frames, trans, np.full(S, -np.inf, dtype=np.float32))
    assert (L == -np.inf).all() and np.isnan(g[np.arange(T)[None, :] < frames[:, None]]).all()
    if not uniform:
        for value in (np.nan, np.inf):
            t2 = trans.copy()
            t2[3, 4] = value
            g, L = device(obs, frames, t2, init)
            assert np.isnan(L).all() and np.isnan(g[np.arange(T)[None, :] < frames[:, None]]).all()
        t2 = np.where(np.eye(S, dtype=bool), trans, -np.inf).astype(np.float32)      # -inf off the diagonal: ordinary zeros
        check(device(obs, frames, t2, init), host(obs, frames, t2, init), frames)


def test_identical_calls_give_identical_bits():
    B, T, S = 70, 30, 1440
    obs, trans, init = synth.problem(B, T, S, seed=12)
    frames = np.clip(synth.lengths(B, 1, T, seed=3), 1, T).astype(np.int32)
    a = device(obs, frames, trans, init)
    b = device(obs, frames, trans, init)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def test_graph_capture_replays_on_new_observations():
    B, T, S = 20, 25, 400
    obs, trans, init = synth.problem(B, T, S, seed=13)
    obs2 = synth.problem(B, T, S, seed=14)[0]
    frames = np.clip(synth.lengths(B, 1, T, seed=5), 1, T).astype(np.int32)
    tobs, tframes, ttrans, tinit = (torch.as_tensor(np.ascontiguousarray(x)).to(DEV) for x in (obs, frames, trans, init))
    ws = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=DEV)
    eager = [x.clone() for x in torbi_amd.forward_backward(tobs, tframes, ttrans, tinit, workspace=ws)]
    eager2 = [x.clone() for x in torbi_amd.forward_backward(torch.as_tensor(obs2).to(DEV), tframes, ttrans, tinit,
                                                            workspace=ws)]
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            post, loglik = torbi_amd.forward_backward(tobs, tframes, ttrans, tinit, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(post, eager[0]) and torch.equal(loglik, eager[1])
    tobs.copy_(torch.as_tensor(obs2))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(post, eager2[0]) and torch.equal(loglik, eager2[1])


def test_likelihood_is_at_least_the_best_path_score():
    B, T, S = 16, 40, 200
    obs, trans, init = synth.problem(B, T, S, seed=15)
    frames = np.clip(synth.lengths(B, 1, T, seed=6), 1, T).astype(np.int32)
    clamped = torch.as_tensor(obs).clone()
    torch.exp_(clamped)
    clamped += torch.finfo(torch.float32).tiny
    torch.log_(clamped)
    _, last = oracle.decode(clamped.numpy(), frames, trans, init, return_posterior=True)
    best = last.astype(np.float64).max(axis=1)
    _, L = device(obs, frames, trans, init)
    assert np.all(L >= best - (1e-6 * np.abs(best) + 4e-6 * frames))


@pytest.mark.parametrize('S', [1441, 4096])
def test_uniform_route_unaligned_and_long_rows(S):
    """Rows the uniform kernel cannot hold in registers: S % 4 != 0 (one float at a time) and S > 2048 (three passes)."""
    B, T = 5, 12
    obs, _, init = synth.problem(B, T, S, seed=S)
    frames = np.array([12, 1, 7, 12, 3], dtype=np.int32)
    check(device(obs, frames, None, init), host(obs, frames, None, init), frames)


@pytest.mark.parametrize('uniform', [False, True])
def test_more_items_than_one_grid_dimension_holds(uniform):
    """70 000 items: more than 65 535 workgroups along the item axis of the per-item kernels."""
    B, T, S = 70000, 3, 5
    obs, trans, init = synth.problem(B, T, S, seed=21)
    frames = np.clip(synth.lengths(B, 1, T, seed=9), 1, T).astype(np.int32)
    trans = None if uniform else trans
    check(device(obs, frames, trans, init), host(obs, frames, trans, init), frames)
