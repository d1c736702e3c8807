"""What tests/test_max_marginals_cpu.py and tests/test_max_marginals_gpu.py share: the two references of the max-marginal
contract, written here independently of torbi_amd/margins.py, the generators of their inputs, the comparison, and the
operand-form rows of the two entries.

The contract (MARGINALS.md), all sums float32 with one rounding each, A indexed [next, prev], F clamped to [1, T]:

    alpha_0 = fl(o_0 + pi);  alpha_t[j] = fl(o_t[j] + max_i fl(alpha_{t-1}[i] + A[j, i]))
    beta_{F-1} = +0;         beta_t[i] = max_j fl(A[j, i] + fl(o_{t+1}[j] + beta_{t+1}[j]))
    m_t = fl(alpha_t + beta_t) for t < F, -inf beyond;  score = max_j alpha_{F-1}[j]

`loop` is that in numpy float32, item by item.  `brute` enumerates all S^F paths of an item in float64.  On DYADIC inputs --
multiples of 1/8 in [-8, 0], at most 6 frames -- every float32 sum is exact (a path's score is a multiple of 1/8 above -104),
so the float32 result must equal the float64 enumeration exactly, and max_j m_t[j] == score for every t < F.

A maximum of floats without NaN does not depend on its order: the values are compared with `==` (so -0 equals +0, the one
thing the contract leaves open) and the NaN positions separately.
"""
import functools
import itertools
import math

import numpy as np
import torch

import operand_form_cases as ofc
from torbi_amd import margins

NINF = np.float32(-np.inf)


def uniform_value(S):
    """The float32 fill of the matrix `transition=None` stands for."""
    return np.float32(math.log(1. / S))


def clamp(frames, T):
    return np.clip(np.asarray(frames, np.int64), 1, T)


def odd(x):
    """NaN or +inf."""
    return ~(np.asarray(x) < np.inf)


def loop(obs, frames, A, pi):
    """(m (B, T, S) float32, score (B,) float32): the contract as a numpy float32 loop.  A = None: the uniform model's filled
    matrix."""
    obs = np.asarray(obs, np.float32)
    pi = np.asarray(pi, np.float32)
    B, T, S = obs.shape
    F = clamp(frames, T)
    A = np.full((S, S), uniform_value(S), np.float32) if A is None else np.asarray(A, np.float32)
    m = np.full((B, T, S), NINF, np.float32)
    score = np.empty((B,), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(B):
            f = int(F[b])
            if odd(obs[b, :f]).any() or odd(pi).any() or (f >= 2 and odd(A).any()):
                m[b, :f] = np.nan
                score[b] = np.nan
                continue
            alpha = np.empty((f, S), np.float32)
            alpha[0] = obs[b, 0] + pi
            for t in range(1, f):
                alpha[t] = obs[b, t] + (alpha[t - 1][None, :] + A).max(axis=1)
            beta = np.zeros((S,), np.float32)
            m[b, f - 1] = alpha[f - 1] + beta
            for t in range(f - 2, -1, -1):
                w = obs[b, t + 1] + beta
                beta = (A + w[:, None]).max(axis=0)
                m[b, t] = alpha[t] + beta
            score[b] = alpha[f - 1].max()
    assert m.dtype == np.float32
    return m, score


def brute(obs, frames, A, pi):
    """(m (B, T, S) float64, score (B,) float64, best (B,) int: how many paths reach the score): every path of every item,
    summed in float64.  Inputs without NaN or +inf."""
    obs = np.asarray(obs, np.float64)
    pi = np.asarray(pi, np.float64)
    B, T, S = obs.shape
    F = clamp(frames, T)
    A = np.full((S, S), np.float64(uniform_value(S))) if A is None else np.asarray(A, np.float64)
    m = np.full((B, T, S), -np.inf)
    score = np.full((B,), -np.inf)
    best = np.zeros((B,), np.int64)
    for b in range(B):
        f = int(F[b])
        for path in itertools.product(range(S), repeat=f):
            value = pi[path[0]] + obs[b, 0, path[0]]
            for t in range(1, f):
                value = value + A[path[t], path[t - 1]] + obs[b, t, path[t]]
            for t in range(f):
                m[b, t, path[t]] = max(m[b, t, path[t]], value)
            if value > score[b]:
                score[b], best[b] = value, 1
            elif value == score[b]:
                best[b] += 1
    return m, score, best


def dyadic(B, T, S, seed, holes=0.):
    """(obs, A, pi) float32, multiples of 1/8 in [-8, 0]; with `holes`, that share of the matrix's entries is -inf, and so are
    A[0, S - 1] and the start in state S - 1 where there is more than one state."""
    rng = np.random.default_rng(seed)
    draw = lambda *shape: (rng.integers(-64, 1, size=shape) / 8.).astype(np.float32)
    obs, A, pi = draw(B, T, S), draw(S, S), draw(S)
    if holes:
        A[rng.random((S, S)) < holes] = NINF
        if S > 1:
            pi[S - 1] = A[0, S - 1] = NINF
    return obs, A, pi


def ragged(B, T, seed):
    """Lengths in 1 .. T; item 0 has T frames and, where there is a second item, the last has 1."""
    frames = np.random.default_rng(seed).integers(1, T + 1, size=B).astype(np.int32)
    frames[0] = T
    if B >= 2:
        frames[B - 1] = 1
    return frames


@functools.lru_cache(maxsize=None)
def dyadic_case(B, T, S, seed, holes):
    """(obs, frames, A, pi, the brute-force (m, score, best)) of a dyadic problem: computed once, never written."""
    obs, A, pi = dyadic(B, T, S, seed, holes)
    frames = ragged(B, T, seed)
    return obs, frames, A, pi, brute(obs, frames, A, pi)


# (S, T) of every dyadic case: S in 1 .. 3, T in 1 .. 5, and one of 6 frames; with holes: a matrix with -inf entries
DYADIC = [(S, T, holes) for S in (1, 2, 3) for T in (1, 2, 3, 4, 5) for holes in (0., .3)] + [(3, 6, 0.), (3, 6, .3)]
DYADIC_ITEMS = 4


@functools.lru_cache(maxsize=None)
def softmax_case(B, T, S, seed, scale=3., matrix=True):
    """(obs, frames, A or None, pi, loop's (m, score)) of random log-softmax inputs: computed once, never written."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.log_softmax(scale * torch.randn(B, T, S, generator=g), 2).numpy()
    A = torch.log_softmax(scale * torch.randn(S, S, generator=g), 0).numpy() if matrix else None
    pi = torch.log_softmax(torch.randn(S, generator=g), 0).numpy()
    frames = ragged(B, T, seed)
    return obs, frames, A, pi, loop(obs, frames, A, pi)


def same(got, want, what=''):
    """(m, score) of `got` equal `want`'s by value, NaN where and only where `want` has NaN.  `want` may be float64 (the
    enumeration on dyadic inputs, which float32 holds exactly)."""
    for name, g, w in zip(('marginals', 'score'), got[:2], want[:2]):
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        w = np.asarray(w)
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name, 'NaN positions differ')
        ok = ~np.isnan(w)
        differ = np.flatnonzero(g[ok].astype(np.float64) != w[ok].astype(np.float64))
        assert differ.size == 0, (what, name, f'{differ.size} of {int(ok.sum())} values differ', g[ok][differ[:4]], w[ok][differ[:4]])


def check_path_consistency(got, frames, what=''):
    """Where every sum is exact: max_j m_t[j] == score for every t < F."""
    m, score = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in got[:2])
    F = clamp(frames, m.shape[1])
    for b in range(m.shape[0]):
        assert (m[b, :F[b]].max(axis=1) == score[b]).all(), (what, b)
        assert (m[b, F[b]:] == NINF).all(), (what, b)


def tensors(*arrays, device='cpu'):
    return [None if a is None else torch.from_numpy(np.array(a)).to(device) for a in arrays]


# the two entries as rows of tests/operand_form_cases.py's table (they are not in torbi_amd.__all__, so the table itself has
# no row for them): `forward_backward_max` takes its operands where the observation lives, `max_marginals` has a gpu=None route
ENTRIES = [
    ofc.Entry('forward_backward_max', [], ofc.OFAP, 'dense',
              lambda o, gpu: margins.forward_backward_max(o[ofc.O], o[ofc.F], o[ofc.A], o[ofc.PI]), cpu=True),
    ofc.Entry('max_marginals', [], ofc.OFAP, 'band',
              lambda o, gpu: margins.max_marginals(o[ofc.O], batch_frames=o[ofc.F], transition=o[ofc.A], initial=o[ofc.PI],
                                                   log_probs=True, gpu=gpu), cpu=True),
]
ENTRY = {e.name: e for e in ENTRIES}


def form_cases(device):
    """(entry name, operand, form) of every non-plain case of the two entries on `device`."""
    return [(e.name, operand, name) for e in ENTRIES for operand in e.operands for name in e.forms(operand, device)
            if name != 'plain']
