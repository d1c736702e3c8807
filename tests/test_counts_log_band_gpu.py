"""The log-space band counts on an MI355X (csrc/counts_log_band.hpp, torbi_amd.forward_backward_counts_log_banded and
`arithmetic='log'` of torbi_amd.expected_counts / log_likelihood) against a float64 log-space reference on the FULL matrix,
gathered along the band's diagonals.  Bounds: tests/test_counts_band_gpu.py::check_counts and tests/test_posterior_gpu.py::check.
"""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, inputs
from test_counts_band_gpu import check_counts, gather, to_dev
from test_posterior_band_gpu import DEV, NINF
from test_posterior_log_band_gpu import WIDE_RANGE, check, problem

pytestmark = pytest.mark.gpu

# B, T, S, reach_left, reach_right, background
CASES = [(1, 1, 8, 1, 1, NINF),                    # no pairs: X = 0
         (3, 40, 64, 2, 5, NINF),                  # asymmetric reaches
         (3, 40, 64, 5, 2, -20.0),                 # ... swapped, a finite background: in-band counts only
         (9, 12, 37, 36, 36, -3.0),                # the band clipped to the whole matrix
         (5, 8, 1441, 12, 12, NINF),               # odd S, a ragged last quad
         (2, 30, 300, 87, 87, NINF),               # 175 diagonals: two chunks of diagonals, every wave
         (2, 4, 4096, 255, 256, NINF),             # W = 512
         (515, 3, 65, 2, 1, NINF),                 # G = 2 and a partial tile
         (40, 70, 72, 40, 30, NINF)]               # many shares of the K rows
IDS = lambda c: 'x'.join(map(str, c[:3])) + f'-{c[3]}-{c[4]}-{c[5]:.0f}'


def log_space_counts(obs, frames, trans, init, reach_left, reach_right, weights=None):
    """(gamma, L, band counts, initial counts) in float64 log space with plain torch ops, where `obs` is."""
    o, F, A, pi = (a if torch.is_tensor(a) else to_dev(a) for a in (obs, frames, trans, init))
    o, A, pi = o.double(), A.double(), pi.double()
    B, T, S = o.shape
    F = F.long().clamp(1, T)
    g = torch.ones(B, dtype=torch.float64, device=o.device) if weights is None else torch.as_tensor(weights).double().to(o.device)
    la, lb = torch.empty_like(o), torch.zeros_like(o)
    la[:, 0] = pi + o[:, 0]
    for t in range(1, T):
        la[:, t] = o[:, t] + torch.logsumexp(A[None] + la[:, t - 1, None, :], 2)
    for t in range(T - 2, -1, -1):
        step = torch.logsumexp(A.T[None] + (o[:, t + 1] + lb[:, t + 1])[:, None, :], 2)
        lb[:, t] = torch.where((t < F - 1)[:, None], step, torch.zeros_like(step))
    L = torch.logsumexp(la[torch.arange(B, device=o.device), F - 1], 1)
    X = torch.zeros_like(A)
    for t in range(1, T):
        xi = torch.exp(la[:, t - 1, None, :] + A[None] + (o[:, t] + lb[:, t] - L[:, None])[:, :, None])
        X += torch.where((t < F)[:, None, None], g[:, None, None] * xi, torch.zeros_like(xi)).sum(0)
    valid = (torch.arange(T, device=o.device)[None, :] < F[:, None])[..., None]
    gamma = torch.where(valid, torch.exp(la + lb - L[:, None, None]), torch.zeros_like(o))
    I = (g[:, None] * gamma[:, 0]).sum(0)
    return gamma.cpu().numpy(), L.cpu().numpy(), gather(X.cpu().numpy(), reach_left, reach_right), I.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(*case):
    return log_space_counts(*problem(*case), case[3], case[4])


def device(obs, frames, trans, init, reach_left, reach_right, background, weights=None, workspace=None):
    w = None if weights is None else torch.as_tensor(weights, dtype=torch.float32).to(DEV)
    return torbi_amd.forward_backward_counts_log_banded(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), reach_left,
                                                        reach_right, background, item_weights=w, workspace=workspace)


def f64(x):
    return x.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('case', CASES + WIDE_RANGE, ids=IDS)
def test_against_float64_log_space(case):
    B, T, S, left, right, background = case
    obs, frames, trans, init = problem(*case)
    if B == 515:
        assert _lib.load().torbi_hip_forward_backward_log_band_tile(B, S, left, right, 0) == 2
    if B == 40:                                     # more shares than items: item 0, of T frames, spans two
        assert _lib.load().torbi_hip_forward_backward_counts_log_band_shares(*case[:5]) > B >= 2
    post, L, X, I = device(obs, frames, trans, init, left, right, background)
    rg, rL, rX, rI = reference(*case)
    assert np.isfinite(rL).all()
    check((f64(post), f64(L)), (rg, rL), frames)
    check_counts(X, I, rX, rI, frames, T, IDS(case))
    assert X.shape == rX.shape and not f64(X)[gather(np.ones((S, S)), left, right) == 0].any()      # clipped: exactly 0
    assert T > 1 or not X.any()


@pytest.mark.parametrize('case', [CASES[2], CASES[7]], ids=IDS)
def test_posterior_and_likelihood_are_the_posterior_route_s_bits(case):
    obs, frames, trans, init = problem(*case)
    post, L = device(obs, frames, trans, init, *case[3:])[:2]
    post2, L2 = torbi_amd.forward_backward_log_banded(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), *case[3:])
    assert torch.equal(post, post2) and torch.equal(L, L2)


def test_workspace_repeatability_and_skipping():
    case = CASES[7]                                 # G = 2: item 3 (NaN) shares its tile with item 2, item 5 (weight 0) with 4
    B, T, S, left, right, background = case
    obs, frames, trans, init = problem(*case)
    frames = np.array(frames)
    frames[2:6] = T                                 # (the NaN below has to be inside its item's frames)
    bad = np.array(obs)
    bad[3, 1, 7] = math.nan                         # L_3 = NaN
    g = np.random.default_rng(4).uniform(0.5, 1.5, size=B).astype(np.float32)
    g[5] = 0.
    ws = torch.full((torbi_amd.expected_counts_log_banded_workspace_bytes(*case[:5]),), 0xFF, dtype=torch.uint8, device=DEV)
    post, L, X, I = device(bad, frames, trans, init, left, right, background, g, workspace=ws)
    assert math.isnan(L[3].item()) and torch.isfinite(L[5]) and torch.isfinite(X).all() and torch.isfinite(I).all()
    for again in (device(bad, frames, trans, init, left, right, background, g),
                  device(bad, frames, trans, init, left, right, background, g, workspace=ws)):
        assert all(torch.allclose(a, b, rtol=0, atol=0, equal_nan=True) for a, b in zip(again, (post, L, X, I)))   # (item 3 is NaN)
    keep = np.delete(np.arange(B), [3, 5])
    Xk, Ik = device(obs[keep], frames[keep], trans, init, left, right, background, g[keep])[2:]
    check_counts(X, I, f64(Xk), f64(Ik), frames[keep], T, 'two items fewer')
    assert torch.equal(device(bad, frames, trans, init, left, right, background, -g)[2], -X)


def test_a_broken_promise_is_nan():
    case = CASES[1]
    obs, frames, trans, init = problem(*case)
    stray = np.array(trans)
    stray[60, 3] = -1.0                             # outside the stated band, not `background`
    post, L, X, I = device(obs, frames, stray, init, *case[3:])
    assert torch.isnan(L).all() and torch.isnan(X).all() and torch.isnan(I).all()


def test_expected_counts_takes_the_route_where_the_scaled_one_fails():
    case = WIDE_RANGE[0]
    B, T, S, left, right, _ = case
    obs, frames, trans, init = (torch.from_numpy(np.array(a)) for a in problem(*case))
    prepared, _, init_d = inputs.model(trans, init, True, S, DEV)                      # the model and the observation it ran on
    _, _, rX, rI = log_space_counts(inputs.observation(obs, True, DEV), frames.to(DEV), prepared, init_d, left, right)
    run = lambda arithmetic: torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0, route='band',
                                                       arithmetic=arithmetic)
    X, I, L = run('log')
    check_counts(torch.from_numpy(gather(f64(X), left, right)), I, rX, rI, frames.numpy(), T, 'log')
    X, I, L = run('scaled')
    with pytest.raises(AssertionError):
        check_counts(torch.from_numpy(gather(f64(X), left, right)), I, rX, rI, frames.numpy(), T, 'scaled')


def test_log_likelihood_backward_is_the_operator():
    case = WIDE_RANGE[0]
    obs, frames, trans, init = (to_dev(a) for a in problem(*case))
    leaves = [a.clone().requires_grad_() for a in (obs, trans, init)]
    L = torbi_amd.log_likelihood(leaves[0], frames, leaves[1], leaves[2], route='band', arithmetic='log')
    L.sum().backward()
    post, L2, Xb, I = torbi_amd.forward_backward_counts_log_banded(obs, frames, trans, init, *case[3:])
    assert torch.equal(L.detach(), L2) and torch.equal(leaves[0].grad, post) and torch.equal(leaves[2].grad, I)
    assert torch.equal(leaves[1].grad, torbi_amd.band_counts_to_dense(Xb, case[3], case[4]))
