"""Path statistics without a device (torbi_amd/paths.py, PATHS.md): the host route against the per-path Python loop of
tests/path_cases.py -- scores bit for bit, counts by == --, void paths, -inf and NaN on a path and off it, the round trips
through `best_paths`, `from_probabilities` and `max_marginals`, the sums and the weights of the counts, the gradients of
`best_path_score` and the C-ABI surface.  tests/test_paths_gpu.py runs the device route against the same loop."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, margins, paths

import max_marginal_cases as mmc
import path_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('torbi_hip_path_statistics_workspace_size', 'torbi_hip_path_statistics')
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 2, 130, 65), (5, 2, 9, 3)]              # (B, K, T, S)


def host(obs, frames, A, pi, indices, weights=None, counts=True):
    return paths.path_statistics(*pc.tensors(obs, frames, A, pi, indices, weights), counts=counts)


# ------------------------------------------------------------------------------------------------ against the loop
@pytest.mark.parametrize('B,K,T,S', SHAPES)
@pytest.mark.parametrize('matrix', [True, False], ids=['matrix', 'uniform'])
def test_host_route_equals_the_loop(B, K, T, S, matrix):
    obs, frames, A, pi, indices, (scores, X, I, kept) = pc.case(B, K, T, S, 11 * S + T, matrix)
    if B >= 4:
        assert [int(f) for f in frames[:4]] == [T, 0, 1, T + 5]                 # clamped to 1, 1 frame, all, beyond
    got = host(obs, frames, A, pi, indices)
    assert len(kept) == B * K and np.isfinite(scores).all()
    pc.same_scores(got[0], scores, (B, K, T, S))
    pc.same_counts(got[1:], (X, I), (B, K, T, S))
    only = host(obs, frames, A, pi, indices, counts=False)
    assert only[1] is None and only[2] is None
    pc.same_scores(only[0], scores)


def test_one_path_per_item_and_int64_indices():
    obs, frames, A, pi, indices, (scores, X, I, _) = pc.case(2, 3, 5, 7, 82)
    flat = host(obs, frames, A, pi, indices[:, 1])
    assert flat[0].shape == (2,)
    pc.same_scores(flat[0], scores[:, 1])
    wide = host(obs, frames, A, pi, indices.astype(np.int64))
    pc.same_scores(wide[0], scores)
    pc.same_counts(wide[1:], (X, I))


def test_minus_inf_and_nan_matter_on_the_path_and_nowhere_else():
    obs, frames, A, pi, q = pc.special_case()
    want, X, I, kept = pc.loop(obs, frames, A, pi, q)
    assert want[0, 0] == pc.NINF and np.isnan(want[0, 1]) and np.isnan(want[0, 2]) and np.isfinite(want[0, 3])
    assert len(kept) == 4                                       # a NaN score is no void path: all four are counted
    got = host(obs, frames, A, pi, q)
    pc.same_scores(got[0], want)
    pc.same_counts(got[1:], (X, I))


@pytest.mark.parametrize('bad', [-1, 7, 2 ** 31 - 1, -2 ** 31])
def test_void_paths(bad):
    """An index outside [0, S) at a column < F voids the path; at a column >= F it is ignored."""
    obs, _, A, pi, indices, _ = pc.case(2, 3, 5, 7, 82)
    frames = np.array([3, 5], np.int32)
    q = np.array(indices)
    q[0, 0, 2] = bad                        # the last column item 0 reads: void
    q[0, 1, 3] = bad                        # behind item 0's frames: ignored
    q[1, 2, 0] = bad                        # the first column: void
    want, X, I, kept = pc.loop(obs, frames, A, pi, q)
    assert sorted(set((b, k) for b in range(2) for k in range(3)) - set(kept)) == [(0, 0), (1, 2)]
    assert want[0, 0] == pc.NINF and want[1, 2] == pc.NINF and np.isfinite(want[0, 1])
    got = host(obs, frames, A, pi, q)
    pc.same_scores(got[0], want)
    pc.same_counts(got[1:], (X, I))
    clean = np.array(q)
    clean[0, 1, 3] = 0
    assert torch.equal(host(obs, frames, A, pi, clean)[0], got[0])
    counted = paths.count_paths(torch.from_numpy(q), 7, torch.from_numpy(frames))
    pc.same_counts(counted, (X, I))


# ------------------------------------------------------------------------------------------------ round trips
def _probabilities(B, T, S, seed, matrix=True):
    g = torch.Generator().manual_seed(seed)
    obs = torch.softmax(2. * torch.randn(B, T, S, generator=g), 2)
    A = torch.softmax(2. * torch.randn(S, S, generator=g), 0) if matrix else None
    pi = torch.softmax(torch.randn(S, generator=g), 0)
    return obs, A, pi


@pytest.mark.parametrize('matrix', [True, False], ids=['matrix', 'uniform'])
def test_scoring_best_paths_gives_its_scores_at_every_rank(matrix):
    obs, A, pi = _probabilities(4, 6, 3, 3, matrix)
    frames = torch.tensor([6, 1, 3, 2], dtype=torch.int32)            # item 1 has 3 < 4 paths: a -inf rank of -1 indices
    indices, scores = torbi_amd.best_paths(obs, 4, frames, A, pi, gpu=None)
    assert scores[1, 3] == -math.inf and (indices[1, 3] == -1).all() and torch.isfinite(scores[0]).all()
    got = paths.score_paths(obs, indices, frames, A, pi, gpu=None)
    pc.same_scores(got, scores.numpy())


def test_the_decoded_path_scores_what_best_paths_and_max_marginals_say():
    obs, A, pi = _probabilities(5, 40, 9, 4)
    frames = torch.tensor([40, 1, 17, 40, 2], dtype=torch.int32)
    path = torbi_amd.from_probabilities(obs.clone(), frames, A, pi, gpu=None)
    got = paths.score_paths(obs, path, frames, A, pi, gpu=None)
    assert got.shape == (5,)
    _, best = torbi_amd.best_paths(obs, 1, frames, A, pi, gpu=None)
    _, score = margins.max_marginals(obs, frames, A, pi, gpu=None)
    pc.same_scores(got, best[:, 0].numpy())
    pc.same_scores(got, score.numpy())
    X, I, again = paths.viterbi_counts(obs, frames, A, pi, gpu=None)
    pc.same_scores(again, best[:, 0].numpy())
    pc.same_counts((X, I), pc.loop(None, frames.numpy(), 9, None, path.numpy()[:, None, :])[1:3])


@pytest.mark.parametrize('S,T,holes', [(2, 5, 0.), (3, 6, 0.), (3, 6, .3)])
def test_on_exact_sums_the_max_marginal_along_the_best_path_is_its_score(S, T, holes):
    obs, frames, A, pi, _ = mmc.dyadic_case(mmc.DYADIC_ITEMS, T, S, 100 * S + T, holes)
    o, f, a, p = mmc.tensors(obs, frames, A, pi)
    m, score = margins.forward_backward_max(o, f, a, p)
    path = torbi_amd.decode_cpu(o, f, a, p)
    got = paths.path_statistics(o, f, a, p, path, counts=False)[0]
    pc.same_scores(got, score.numpy())
    for b in range(len(frames)):
        for t in range(int(mmc.clamp(frames, T)[b])):
            assert m[b, t, path[b, t]] == score[b], (b, t)


# ------------------------------------------------------------------------------------------------ counts
def test_counts_sum_to_the_steps_and_the_paths_that_are_not_void():
    B, K, T, S = 3, 2, 130, 65
    q = np.array(pc.random_paths(B, K, T, S, 3))
    frames = np.array([130, 64, 1], np.int32)
    q[1, 0, 5] = -1
    w = pc.dyadic_weights(B, K, 4)
    X, I = paths.count_paths(*pc.tensors(q, device='cpu'), S, torch.from_numpy(frames), torch.from_numpy(w))
    live = np.ones((B, K), bool)
    live[1, 0] = False
    assert float(I.double().sum()) == float((w.astype(np.float64) * live).sum())
    assert float(X.double().sum()) == float((w.astype(np.float64) * live * (frames[:, None] - 1)).sum())
    pc.same_counts((X, I), pc.weighted(q, frames, S, w))
    X1, I1 = paths.count_paths(torch.from_numpy(q), S, torch.from_numpy(frames))
    assert float(I1.sum()) == 5. and float(X1.sum()) == 2 * 129 + 63 + 0         # (one of item 1's two paths is void)


def test_general_weights_are_within_one_rounding_of_the_float64_loop():
    B, K, T, S = 3, 2, 130, 2                   # two states: every cell receives hundreds of adds
    q = pc.random_paths(B, K, T, S, 9)
    frames = np.array([130, 77, 130], np.int32)
    w = pc.general_weights(B, K, 10)
    got = paths.count_paths(torch.from_numpy(q), S, torch.from_numpy(frames), torch.from_numpy(w))
    pc.same_counts(got, pc.weighted(q, frames, S, w), relative=pc.ULP)


# ------------------------------------------------------------------------------------------------ gradients
def test_best_path_score_gradients_are_the_one_hot_path_and_its_weighted_counts():
    obs, frames, A, pi, _, _ = pc.case(3, 2, 130, 65, 11 * 65 + 130)
    o, f, a, p = pc.tensors(obs, frames, A, pi)
    o, a, p = o.requires_grad_(), a.requires_grad_(), p.requires_grad_()
    score = paths.best_path_score(o, f, a, p)
    g = torch.tensor([1., .5, -2.])
    (score * g).sum().backward()
    path = torbi_amd.decode_cpu(o.detach(), f, a.detach(), p.detach())
    pc.same_scores(score.detach(), pc.loop(obs, frames, A, pi, path.numpy()[:, None, :])[0][:, 0])
    F = pc.clamp(frames, 130)
    want = np.zeros((3, 130, 65), np.float32)
    for b in range(3):
        for t in range(int(F[b])):
            want[b, t, int(path[b, t])] = float(g[b])
    assert np.array_equal(o.grad.numpy(), want)
    X, I = paths.count_paths(path, 65, f, g)
    assert torch.equal(a.grad, X) and torch.equal(p.grad, I)
    # only what is asked for
    o2 = torch.from_numpy(np.array(obs)).requires_grad_()
    paths.best_path_score(o2, f, a.detach(), p.detach()).sum().backward()
    assert o2.grad.sum() == float(F.sum())


# ------------------------------------------------------------------------------------------------ fronts
def test_fronts_and_refusals():
    scores, X, I = paths.path_statistics(torch.empty(0, 3, 4), None, None, torch.zeros(4), torch.empty(0, 2, 3, dtype=torch.int32))
    assert scores.shape == (0, 2) and X.shape == (4, 4) and I.shape == (4,) and float(X.sum()) == 0. == float(I.sum())
    with pytest.raises(RuntimeError, match='initial'):
        paths.path_statistics(torch.zeros(1, 2, 3), None, None, None, torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='indices must have shape'):
        paths.path_statistics(torch.zeros(1, 2, 3), None, None, torch.zeros(3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='int32 or int64'):
        paths.score_paths(torch.rand(1, 2, 3), torch.zeros(1, 2))
    with pytest.raises(RuntimeError, match='path_weights must have shape'):
        paths.count_paths(torch.zeros(2, 3, 4, dtype=torch.int32), 5, path_weights=torch.ones(2))
    obs = torch.rand(2, 4, 3) + .1
    before = obs.clone()
    got = paths.score_paths(obs, torch.zeros(2, 4, dtype=torch.int64))
    assert torch.equal(obs, before) and got.shape == (2,) and torch.isfinite(got).all()      # the defaults; nothing written


# ------------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_surface():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    declared = set(re.findall(r'\b(torbi_hip_\w+)\s*\(', header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert not name.endswith('_bytes')
    assert '#define TORBI_HIP_ABI_VERSION 17' in header
    assert _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert 'paths' in torbi_amd.__all__ and torbi_amd.paths is paths
    assert not set(paths.__all__) & set(torbi_amd.__all__)
    size = lib.torbi_hip_path_statistics_workspace_size
    assert _lib.SYMBOLS[NAMES[0]][0] is ctypes.c_size_t
    assert size(3, 5, 7, 2, 0) == 0 and paths.path_statistics_workspace_bytes(3, 5, 7, 2, counts=False) == 0
    for nonsense in [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 16385, 1)]:
        assert size(*nonsense, 1) == 256, nonsense
    sizes = [size(3, 5, S, 2, 1) for S in (1, 2, 7, 65, 1440)]
    assert sizes == sorted(sizes) and sizes[0] > 256 and sizes[-1] >= 8 * (1440 * 1440 + 1440)
    assert size(3, 5, 65, 2, 1) == size(512, 500, 65, 16, 1) == paths.path_statistics_workspace_bytes(3, 5, 65, 2)


def test_argument_checks_come_before_any_device():
    """Dummy addresses that nothing dereferences and a device index no machine has (tests/test_workspace_alignment_cpu.py):
    a call whose arguments pass ends where it selects its device, with a HIP error code."""
    lib = _lib.load()
    EINVAL, EWORKSPACE, p, dev = -1, -2, 1 << 16, 63
    B, T, S, K = 3, 6, 72, 2
    need = lib.torbi_hip_path_statistics_workspace_size(B, T, S, K, 1)
    u = ctypes.c_float(-4.)
    call = lambda *a: lib.torbi_hip_path_statistics(*a)
    full = lambda ws, n, dims=(B, T, S, K): call(p, p, p, u, p, p, p, p, p, p, ws, n, *dims, dev, None)
    for base in ((1 << 20), (1 << 20) + 1):
        assert full(base, need - 1) == EWORKSPACE
        assert full(base, need) > 0
    assert call(p, p, None, u, p, p, None, p, None, None, None, 0, B, T, S, K, dev, None) > 0       # scores only, uniform
    assert call(None, p, None, u, None, p, None, None, p, p, p, need, B, T, S, K, dev, None) > 0     # counts only, no model
    for dims in [(-1, T, S, K), (B, 0, S, K), (B, T, 0, K), (B, T, S, 0)]:
        assert full(p, need, dims) == EINVAL, dims
    assert call(None, p, p, u, p, p, p, p, p, p, p, need, B, T, S, K, dev, None) == EINVAL           # scores without observation
    assert call(p, p, p, u, None, p, p, p, p, p, p, need, B, T, S, K, dev, None) == EINVAL           # ... without initial
    assert call(p, None, p, u, p, p, p, p, p, p, p, need, B, T, S, K, dev, None) == EINVAL           # no frames
    assert call(p, p, p, u, p, None, p, p, p, p, p, need, B, T, S, K, dev, None) == EINVAL           # no indices
    assert call(p, p, p, u, p, p, p, p, p, None, p, need, B, T, S, K, dev, None) == EINVAL           # one count output
    assert call(p, p, p, u, p, p, p, p, None, p, p, need, B, T, S, K, dev, None) == EINVAL
    assert call(p, p, p, u, p, p, p, None, None, None, p, need, B, T, S, K, dev, None) == EINVAL     # no output at all
    assert call(p, p, p, u, p, p, p, p, p, p, None, need, B, T, S, K, dev, None) == EINVAL           # counts, no workspace
    assert full(p, need, (0, T, S, K)) == 0                                                           # an empty batch
