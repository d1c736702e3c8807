"""The wide band route of the expected counts on an MI355X (csrc/counts_wide_band.hpp, torbi_amd.forward_backward_counts_wide_banded
and the routing of torbi_amd.expected_counts / log_likelihood) against training._host_counts in float64 on the FULL matrix,
gathered along the band's diagonals.  Bounds: tests/test_counts_band_gpu.py::check_counts and tests/test_posterior_gpu.py::check.
"""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, inputs, training
from test_counts_band_gpu import check_counts, gather, to_dev
from test_posterior_wide_band_gpu import DEV, NINF, TINY, check, problem

pytestmark = pytest.mark.gpu

# B, T, S, reach_left, reach_right, background
CASES = [(1, 1, 8, 7, 7, NINF),                    # no pairs: X = 0
         (3, 12, 72, 40, 30, NINF),                # asymmetric: a transposed or mirrored diagonal
         (3, 12, 72, 30, 40, -20.0),               # ... the reaches swapped, a finite background: in-band counts only
         (2, 9, 131, 130, 130, -3.0),              # the band is the whole matrix; odd S, a ragged last quad, windows clipped on both edges
         (5, 8, 1440, 87, 87, NINF),               # the pitch matrix of 175 diagonals, peaked rows: one window chunk
         (5, 8, 1440, 87, 87, TINY),               # ... log(tiny) outside
         (2, 4, 4096, 255, 256, NINF),             # three window chunks
         (515, 3, 68, 40, 33, NINF),               # G = 2 and a partial last tile, ragged frames
         (1030, 3, 68, 40, 33, NINF),              # G = 4 and a partial last tile
         (40, 70, 72, 40, 30, NINF)]               # 44 K blocks in KS = 44 shares of one block: every item spans two or three shares
IDS = lambda c: 'x'.join(map(str, c[:3])) + f'-{c[3]}-{c[4]}-{c[5]:.0f}'


@functools.lru_cache(maxsize=None)
def reference(*case):
    """(gamma, L, band counts, initial counts) of `problem(*case)` in float64, computed once."""
    g, L, X, I = training._host_counts(*(torch.from_numpy(np.array(a)) for a in problem(*case)), None)
    return g.numpy(), L.numpy(), gather(X.numpy(), case[3], case[4]), I.numpy()


def device(obs, frames, trans, init, reach_left, reach_right, background, weights=None, workspace=None):
    w = None if weights is None else torch.as_tensor(weights, dtype=torch.float32).to(DEV)
    out = torbi_amd.forward_backward_counts_wide_banded(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), reach_left,
                                                        reach_right, background, item_weights=w, workspace=workspace)
    S = obs.shape[2]
    assert all(x.device == DEV and x.dtype == torch.float32 for x in out)
    assert out[2].shape == (min(reach_left, S - 1) + min(reach_right, S - 1) + 1, S) and out[3].shape == (S,)
    return out


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_against_float64(case):
    B, T, S, left, right, background = case
    obs, frames, trans, init = problem(*case)
    if B == 40:
        assert _lib.load().torbi_hip_forward_backward_counts_wide_band_shares(*case[:5]) == 44
    post, L, X, I = device(obs, frames, trans, init, left, right, background)
    rg, rL, rX, rI = reference(*case)
    assert np.isfinite(rL).all()
    check((post.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)), (rg, rL), frames)
    check_counts(X, I, rX, rI, frames, T, IDS(case))
    assert not X.cpu().numpy()[gather(np.ones((S, S)), left, right) == 0].any()      # clipped positions are exactly 0
    assert T > 1 or not X.any()


@pytest.mark.parametrize('case', [CASES[2], CASES[8]], ids=IDS)
def test_posterior_and_likelihood_are_the_posterior_route_s_bits(case):
    obs, frames, trans, init = problem(*case)
    post, L = device(obs, frames, trans, init, *case[3:])[:2]
    post2, L2 = torbi_amd.forward_backward_wide_banded(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), *case[3:])
    assert torch.equal(post, post2) and torch.equal(L, L2)


def test_skipping_is_selection():
    case = CASES[7]                                 # G = 2: item 3 (NaN) shares its tile with item 2, item 5 (weight 0) with 4
    B, T, S, left, right, background = case
    obs, frames, trans, init = problem(*case)
    frames = np.array(frames)
    frames[2:6] = T                                 # (the NaN below has to be inside its item's frames; the rest stay ragged)
    bad = np.array(obs)
    bad[3, 1, 7] = math.nan                         # L_3 = NaN
    g = np.random.default_rng(4).uniform(0.5, 1.5, size=B).astype(np.float32)
    g[5] = 0.
    ws = torch.full((torbi_amd.expected_counts_wide_banded_workspace_bytes(*case[:5]),), 0xFF, dtype=torch.uint8, device=DEV)
    post, L, X, I = device(bad, frames, trans, init, left, right, background, g, workspace=ws)
    assert math.isnan(L[3].item()) and torch.isnan(post[3]).all() and torch.isfinite(L[2]) and torch.isfinite(post[2]).all()
    assert torch.isfinite(X).all() and torch.isfinite(I).all()
    own = device(bad, frames, trans, init, left, right, background, g)
    assert torch.equal(X, own[2]) and torch.equal(I, own[3])
    keep = np.delete(np.arange(B), [3, 5])
    Xk, Ik = device(obs[keep], frames[keep], trans, init, left, right, background, g[keep])[2:]
    check_counts(X, I, Xk.cpu().numpy().astype(np.float64), Ik.cpu().numpy().astype(np.float64), frames[keep], T, 'two items fewer')
    X2, I2 = device(bad, frames, trans, init, left, right, background, 2 * g)[2:]
    assert torch.allclose(X2, 2 * X, rtol=1e-6, atol=1e-7 * X.abs().max().item())
    assert torch.allclose(I2, 2 * I, rtol=1e-6, atol=1e-7 * I.abs().max().item())
    assert torch.equal(device(bad, frames, trans, init, left, right, background, -g)[2], -X)


def test_a_broken_promise_and_a_nan_inside_the_band():
    case = CASES[1]
    B, T, S, left, right, background = case
    obs, frames, trans, init = problem(*case)
    F = np.clip(frames, 1, T)
    valid = torch.from_numpy(np.arange(T)[None, :] < F[:, None]).to(DEV)
    stray = np.array(trans)
    stray[60, 3] = -1.0                             # outside the stated band, not `background`
    post, L, X, I = device(obs, frames, stray, init, *case[3:])
    assert torch.isnan(L).all() and torch.isnan(post[valid]).all() and (post[~valid] == 0).all()
    assert torch.isnan(X).all() and torch.isnan(I).all()
    bad = np.array(trans)
    bad[20, 50] = np.nan                            # next 20, prev 50: inside reach_right = 30, diagonal 50 - 20 + 40
    post, L, X, I = device(obs, frames, bad, init, *case[3:])
    assert np.array_equal(torch.isnan(L).cpu().numpy(), F >= 2) and torch.isnan(X[70, 20])


def test_routing():
    """A -inf band of 71 entries at 72 states goes to the wide operator under route='band' (it raised before there was one);
    its share of the row is in no measured class, so 'auto' stays dense.  A band of 40 entries goes where it went."""
    case = CASES[1]
    B, T, S, left, right, _ = case
    obs, frames, trans, init = (torch.from_numpy(np.array(a)) for a in problem(*case))
    prepared, _, init_d = inputs.model(trans, init, True, S, DEV)
    obs_d = inputs.observation(obs, True, DEV)
    X, I, L = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0, route='band')
    _, L2, Xb, I2 = torbi_amd.forward_backward_counts_wide_banded(obs_d, frames, prepared, init_d, left, right)
    assert torch.equal(X, torbi_amd.band_counts_to_dense(Xb, left, right)) and torch.equal(I, I2) and torch.equal(L, L2)
    assert torbi_amd.counts_route(trans, B, T, S, gpu=0, log_probs=True) == 'dense'
    narrow = torch.from_numpy(np.array(problem(3, 12, 72, 20, 19, NINF)[2]))
    prepared, _, _ = inputs.model(narrow, init, True, S, DEV)
    X, I, L = torbi_amd.expected_counts(obs, frames, narrow, init, log_probs=True, gpu=0, route='band')
    _, L2, Xb, I2 = torbi_amd.forward_backward_counts_banded(obs_d, frames, prepared, init_d, 20, 19)
    assert torch.equal(X, torbi_amd.band_counts_to_dense(Xb, 20, 19)) and torch.equal(I, I2) and torch.equal(L, L2)
    # the gradients of log_likelihood(route='band') against the float64 route: the bounds of tests/test_counts_band_gpu.py
    w = torch.as_tensor(np.random.default_rng(2).uniform(0.5, 1.5, B))
    leaves = {}
    for where in ('cpu', 'gpu'):
        args = [a.double() if where == 'cpu' else a.to(DEV) for a in (obs, trans, init)]
        args = [a.requires_grad_() for a in args]
        Lw = torbi_amd.log_likelihood(args[0], frames.to(args[0].device), args[1], args[2], route='band')
        (Lw * w.to(Lw.device, Lw.dtype)).sum().backward()
        leaves[where] = [Lw.detach().cpu().double().numpy()] + [a.grad.cpu().double().numpy() for a in args]
    c, g = leaves['cpu'], leaves['gpu']
    F = np.clip(frames.numpy(), 1, T)
    assert np.all(np.abs(g[0] - c[0]) <= 1e-6 * np.abs(c[0]) + 4e-6 * F)
    assert np.abs(g[1] - c[1]).max() <= 1e-4
    check_counts(torch.as_tensor(g[2]), torch.as_tensor(g[3]), c[2], c[3], F, T, 'gradients, wide band')
