"""What tests/test_paths_cpu.py and tests/test_paths_gpu.py share: the reference of the path-statistics contract (PATHS.md),
written here independently of torbi_amd/paths.py, the generators of their inputs and the comparison.

The contract, A indexed [next, prev], F clamped to [1, T], every sum float32 with one rounding:

    s_0 = fl(o_0[q_0] + pi[q_0]);   s_t = fl(o_t[q_t] + fl(s_{t-1} + A[q_t, q_{t-1}]))   1 <= t < F;   score = s_{F-1}
    X[j, i] = sum w #{1 <= t < F: q_t = j, q_{t-1} = i};   I[j] = sum w [q_0 = j]       (float64 sums, one rounding)

A path with an index outside [0, S) at a column t < F is void: score -inf, no counts.  `loop` is that path by path: the
chain over np.float32 scalars, the counts in dictionaries -- of Python integers where the weights are integers (exact
whatever happens), of Python floats (float64) in the order b, k, t otherwise.
"""
import functools
import math

import numpy as np
import torch

NINF = np.float32(-np.inf)
ULP = 2. ** -23                          # the derived bound on general weights: one float32 rounding of a float64 sum


def uniform_value(S):
    """The float32 fill of the matrix `transition=None` stands for."""
    return np.float32(math.log(1. / S))


def clamp(frames, T):
    return np.clip(np.asarray(frames, np.int64), 1, T)


def loop(obs, frames, A, pi, indices, weights=None, uniform=None):
    """(scores (B, K) float32 or None, X (S, S) float32, I (S,) float32, kept: the (b, k) of the non-void paths).  obs = None:
    counts only (then `A` is the state count S).  A = None with an observation: the uniform model."""
    indices = np.asarray(indices)
    B, K, T = indices.shape
    S = int(A) if obs is None else np.asarray(obs).shape[2]
    F = clamp(frames, T)
    scores = None
    if obs is not None:
        obs, pi = np.asarray(obs, np.float32), np.asarray(pi, np.float32)
        A = None if A is None else np.asarray(A, np.float32)
        u = uniform_value(S) if uniform is None else np.float32(uniform)
        scores = np.empty((B, K), np.float32)
    whole = weights is None or np.issubdtype(np.asarray(weights).dtype, np.integer)
    zero = 0 if whole else 0.
    X, I, kept = {}, {}, []
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(B):
            f = int(F[b])
            for k in range(K):
                q = [int(v) for v in indices[b, k, :f]]
                if any(v < 0 or v >= S for v in q):
                    if scores is not None:
                        scores[b, k] = NINF
                    continue
                kept.append((b, k))
                w = 1 if weights is None else (int(weights[b][k]) if whole else float(weights[b][k]))
                I[q[0]] = I.get(q[0], zero) + w
                for t in range(1, f):
                    X[q[t], q[t - 1]] = X.get((q[t], q[t - 1]), zero) + w
                if scores is None:
                    continue
                s = np.float32(obs[b, 0, q[0]] + pi[q[0]])
                for t in range(1, f):
                    a = u if A is None else A[q[t], q[t - 1]]
                    s = np.float32(obs[b, t, q[t]] + np.float32(s + a))
                assert s.dtype == np.float32
                scores[b, k] = s
    Xd, Id = np.zeros((S, S), np.float64), np.zeros((S,), np.float64)
    for (j, i), v in X.items():
        Xd[j, i] = v
    for j, v in I.items():
        Id[j] = v
    return scores, Xd, Id, kept


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return np.ascontiguousarray(x).view(np.int32)


def same_scores(got, want, what=''):
    """Bit for bit, except that any NaN equals any NaN (the positions must agree)."""
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    w = np.asarray(want)
    assert g.dtype == np.float32 and w.dtype == np.float32 and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, 'NaN positions differ', g, w)
    ok = ~np.isnan(w)
    differ = np.flatnonzero(bits(g)[ok] != bits(w)[ok])
    assert differ.size == 0, (what, f'{differ.size} of {int(ok.sum())} scores differ', g[ok][differ[:4]], w[ok][differ[:4]])


def same_counts(got, want, what='', relative=0.):
    """`got` (X, I) float32 tensors against `want` (X, I) float64 arrays: by == (relative = 0: every count is a float32
    number), or within `relative` of the float64 value."""
    for name, g, w in zip(('transition_counts', 'initial_counts'), got, want):
        g = g.detach().cpu().numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if relative == 0.:
            assert np.abs(w).max(initial=0.) < 2. ** 24 or (w == w.astype(np.float32)).all()
            differ = np.flatnonzero(g.astype(np.float64) != w)
        else:
            differ = np.flatnonzero(np.abs(g.astype(np.float64) - w) > relative * np.abs(w))
        assert differ.size == 0, (what, name, f'{differ.size} cells differ', g.flat[differ[:4]], w.flat[differ[:4]])


def model(B, T, S, seed, matrix=True, scale=3.):
    """(obs, A or None, pi) float32: log-softmax inputs, finite everywhere."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.log_softmax(scale * torch.randn(B, T, S, generator=g), 2).numpy()
    A = torch.log_softmax(scale * torch.randn(S, S, generator=g), 0).numpy() if matrix else None
    pi = torch.log_softmax(torch.randn(S, generator=g), 0).numpy()
    return obs, A, pi


def random_paths(B, K, T, S, seed):
    return np.random.default_rng(seed).integers(0, S, size=(B, K, T)).astype(np.int32)


def frames_of(B, T, seed):
    """Frames that cover 0 (clamped to 1), 1, T and T + 5 where there are items for them; the rest random in 1 .. T."""
    frames = np.random.default_rng(seed).integers(1, T + 1, size=B).astype(np.int32)
    for b, f in zip(range(B), (T, 0, 1, T + 5)[:max(1, B)]):
        frames[b] = f
    return frames


def dyadic_weights(B, K, seed):
    """Multiples of 1/8 in [0, 4]: every partial sum of fewer than 2^40 of them is exact in float64."""
    return (np.random.default_rng(seed).integers(0, 33, size=(B, K)) / 8.).astype(np.float32)


def general_weights(B, K, seed):
    return np.random.default_rng(seed).random((B, K)).astype(np.float32) + np.float32(.25)


def weighted(indices, frames, S, weights):
    """The float64 loop of weighted counts (X, I) -- exact for dyadic weights."""
    _, X, I, _ = loop(None, frames, S, None, indices, np.asarray(weights, np.float64))
    return X, I


@functools.lru_cache(maxsize=None)
def case(B, K, T, S, seed, matrix=True):
    """(obs, frames, A, pi, indices, loop's (scores, X, I, kept)) of a finite problem with random paths: computed once, never
    written."""
    obs, A, pi = model(B, T, S, seed, matrix)
    frames = frames_of(B, T, seed)
    indices = random_paths(B, K, T, S, seed + 1)
    return obs, frames, A, pi, indices, loop(obs, frames, A, pi, indices)


def special_case(S=7, T=9, seed=5):
    """One item of T frames, S >= 3 states, four paths; -inf and NaN cells on path 0 / 1 and off every path, and a +inf that
    meets a -inf on path 2 (NaN by IEEE).  Returns (obs, frames, A, pi, indices)."""
    obs, A, pi = (np.array(x) for x in model(1, T, S, seed))
    q = np.zeros((1, 4, T), np.int32)
    q[0, 0] = np.arange(T) % 2                      # states 0, 1, 0, 1, ...
    q[0, 1] = 2
    q[0, 2] = np.arange(T) % 2 + 3 if S >= 5 else 2
    q[0, 3] = S - 1
    obs[0, 3, 1] = NINF                             # on path 0: its score is -inf
    obs[0, 4, 2] = np.nan                           # on path 1: NaN
    A[2, 0] = np.nan                                # never taken: paths 0 and 3 do not see it
    obs[0, 5, S - 2] = np.nan if S - 2 > 4 else obs[0, 5, S - 2]      # off every path
    if S >= 5:
        obs[0, 2, 3] = np.inf                       # path 2 at t = 2 ...
        obs[0, 6, 3] = NINF                         # ... and at t = 6: +inf + -inf = NaN
    return obs, np.array([T], np.int32), A, pi, q


def tensors(*arrays, device='cpu'):
    return [None if a is None else torch.from_numpy(np.array(a)).to(device) for a in arrays]
