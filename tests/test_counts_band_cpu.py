"""What the band counts route (csrc/counts_band.hpp, torbi_amd.forward_backward_counts_banded) answers without a device:
coverage, workspace bytes, the layout of its result and the checks of the public arguments."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import posterior, training

NINF = -math.inf
P = 512                                            # planes of a call at most (counts_band.hpp kCountsWorkgroups)


def test_the_new_names_are_exported():
    for name in ('forward_backward_counts_banded', 'expected_counts_banded_workspace_bytes', 'band_counts_to_dense',
                 'counts_route'):
        assert name in torbi_amd.__all__ and callable(getattr(torbi_amd, name))


def test_coverage_is_answered_without_a_device():
    covered = posterior._counts_covered
    assert covered(512, 500, 1440, 11, 11, NINF)                  # the pitch band: 23 x 1440 x 4 B + the rows = 144 KB
    assert covered(512, 500, 1440, 11, 11, math.log(np.finfo(np.float32).tiny))
    assert covered(4, 10, 4096, 3, 3, NINF)                       # 7 x 4096 x 4 B + the rows = 147 KB
    assert not covered(4, 10, 4096, 4, 4, NINF)                   # 9 diagonals: 180 KB
    assert not covered(2, 4, 4096, 31, 32, NINF)                  # 64 diagonals of 4096 states: the posterior route's limit
    assert posterior._covered(2, 4, 4096, 31, 32, NINF)           # ... which that route takes
    assert not covered(8, 60, 1440, 13, 13, NINF)                 # 27 x 1440 x 4 B = 155.5 KB + 11.9 KB of rows
    assert covered(8, 60, 1440, 12, 12, NINF)
    assert covered(9, 12, 37, 36, 36, -3.0)                       # reaches clamped to S - 1
    # whatever the posterior band route refuses
    assert not covered(3, 4, 130, 32, 32, NINF)
    assert not covered(3, 40, 64, 2, 5, math.nan) and not covered(3, 40, 64, 2, 5, math.inf)
    assert not covered(0, 4, 64, 1, 1, NINF) and not covered(3, 4, 64, -1, 1, NINF) and not covered(3, 4, 4097, 1, 1, NINF)


def test_workspace_is_the_band_routes_plus_at_most_p_planes():
    T, S, left, right = 7, 1440, 11, 11
    plane = (left + right + 1) * 1472 * 4                         # [W][S up to 64] fp32
    extra = []
    for B in (1, 2, 3, 100, P - 1, P, P + 1, 4 * P):
        total = torbi_amd.expected_counts_banded_workspace_bytes(B, T, S, left, right)
        band = torbi_amd.forward_backward_banded_workspace_bytes(B, T, S, left, right)
        extra.append(total - band)
        assert min(B, P) * plane <= extra[-1] < min(B, P) * plane + 256
    assert extra == sorted(extra) and extra[0] < extra[1] < extra[2] and extra[-3] == extra[-2] == extra[-1]
    totals = [torbi_amd.expected_counts_banded_workspace_bytes(B, T, S, left, right) for B in range(1, 40)]
    assert totals == sorted(totals)


@pytest.mark.parametrize('S,left,right', [(16, 2, 5), (16, 5, 2), (9, 0, 0), (7, 3, 0), (6, 5, 5), (5, 9, 2)])
def test_band_counts_to_dense_round_trips(S, left, right):
    rng = np.random.default_rng(S + 10 * left + right)
    dense = rng.uniform(1., 2., size=(S, S)).astype(np.float32)
    cl, cr = min(left, S - 1), min(right, S - 1)
    W = cl + cr + 1
    band = np.full((W, S), 7., dtype=np.float32)                 # (clipped positions: whatever, they are dropped)
    inside = np.zeros((S, S), dtype=bool)
    for k in range(W):
        for j in range(S):
            i = j - cl + k
            if 0 <= i < S:
                band[k, j] = dense[j, i]
                inside[j, i] = True
    got = torbi_amd.band_counts_to_dense(torch.from_numpy(band), left, right).numpy()
    assert got.shape == (S, S) and got.dtype == np.float32
    assert np.array_equal(got, np.where(inside, dense, np.float32(0)))
    j, i = np.nonzero(inside)
    assert np.all((i >= j - left) & (i <= j + right))            # [next, prev]: prev within [next - left, next + right]


def test_band_counts_to_dense_checks_the_rows():
    with pytest.raises(RuntimeError, match='rows'):
        torbi_amd.band_counts_to_dense(torch.zeros((4, 16)), 2, 2)


def test_route_values_are_validated():
    obs = torch.zeros((2, 3, 4))
    trans, init = torch.zeros((4, 4)), torch.zeros(4)
    assert training.ROUTES == ('auto', 'dense', 'band')
    with pytest.raises(RuntimeError, match='route must be'):
        torbi_amd.expected_counts(obs, None, trans, init, log_probs=True, route='banded')
    with pytest.raises(RuntimeError, match='route must be'):
        torbi_amd.log_likelihood(obs, None, trans, init, route='fast')
    # the CPU routes ignore a valid one
    a = torbi_amd.expected_counts(obs, None, trans, init, log_probs=True)
    for route in training.ROUTES:
        b = torbi_amd.expected_counts(obs, None, trans, init, log_probs=True, route=route)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(torbi_amd.log_likelihood(obs, None, trans, init, route=route),
                           torbi_amd.log_likelihood(obs, None, trans, init))
    assert torbi_amd.counts_route(trans, 2, 3, 4, gpu=None) == 'dense' and torbi_amd.counts_route(None, 2, 3, 4) == 'dense'
