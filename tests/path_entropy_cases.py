"""What tests/test_path_entropy_cpu.py and tests/test_path_entropy_gpu.py share: three float64 references of the path entropy,
written here independently of torbi_amd/entropy.py, the makers of their inputs, the bounds and the operand-form rows of the
two entries.

The contract (ENTROPY.md): log space, A indexed [next, prev], F clamped to [1, T], -inf a zero probability, a path's weight
exp(pi[q_0] + o_0[q_0] + sum_t (A[q_t, q_{t-1}] + o_t[q_t])) normalised by exp(L);  H = - sum_q P(q) log P(q) in nats;
prefix_t is H of the first t + 1 frames alone.

1. `enumerate_paths`: every one of the S^F paths of an item, in numpy float64 (S^T <= 1024).
2. `loop`: the forward-only recursion of the contract as a plain numpy float64 loop, item by item.
3. `identity`: H = L - (gamma_0 . pi + sum_t gamma_t . o_t + sum_ji X[j, i] A[j, i]) from the posteriors gamma and the expected
   transition counts X of one item, cells of count 0 skipped.  gamma and X come from forward-BACKWARD, another algorithm, so an
   error that the first two references could share shows here.  `state_posteriors` and `expected_counts` round what they
   return to float32, which would lose this difference of two large numbers: the float64 route behind their `gpu=None`
   (`posterior._host`) is called itself, item by item.

Between these float64 references the bound is REFERENCE_RTOL * (1 + |H|): a few thousand float64 operations of relative
error 1.1e-16 each, on sums whose terms can be 1e3 times the result.
"""
import functools
import itertools
import math

import numpy as np
import torch

import operand_form_cases as ofc
from torbi_amd import entropy, posterior

REFERENCE_RTOL = 1e-9
# POSTERIOR.md's bound of the log-likelihood against float64: RTOL_L |ref| + ATOL_L_PER_FRAME F
RTOL_L, ATOL_L_PER_FRAME = 1e-6, 4e-6


def clamp(frames, T):
    return np.clip(np.asarray(frames, np.int64), 1, T)


def uniform_value(S):
    """The float32 fill of the matrix `transition=None` stands for."""
    return np.float32(math.log(1. / S))


def filled(S):
    return np.full((S, S), uniform_value(S), np.float32)


def _f64(obs, A, pi):
    obs = np.asarray(obs, np.float64)
    S = obs.shape[-1]
    return obs, (np.asarray(filled(S), np.float64) if A is None else np.asarray(A, np.float64)), np.asarray(pi, np.float64)


def enumerate_paths(obs, frames, A, pi):
    """(H (B,), L (B,), prefix (B, T)) float64 from every path of every item and of every one of its prefixes."""
    obs, A, pi = _f64(obs, A, pi)
    B, T, S = obs.shape
    F = clamp(frames, T)
    H, L, prefix = np.zeros(B), np.zeros(B), np.zeros((B, T))
    with np.errstate(divide='ignore', invalid='ignore'):
        for b in range(B):
            for f in range(1, int(F[b]) + 1):
                paths = np.array(list(itertools.product(range(S), repeat=f)))                # (S^f, f)
                score = pi[paths[:, 0]] + obs[b, 0, paths[:, 0]]
                for t in range(1, f):
                    score = score + A[paths[:, t], paths[:, t - 1]] + obs[b, t, paths[:, t]]
                top = score.max()
                total = top + np.log(np.exp(score - top).sum())
                logp = score - total
                live = np.isfinite(logp)
                prefix[b, f - 1] = -(np.exp(logp[live]) * logp[live]).sum()
            H[b], L[b] = prefix[b, F[b] - 1], total
    return H, L, prefix


def loop(obs, frames, A, pi):
    """(H, L, prefix) float64: the recursion of the contract, item by item, frame by frame.  Finite-or--inf inputs of
    positive total probability."""
    obs, A, pi = _f64(obs, A, pi)
    B, T, S = obs.shape
    F = clamp(frames, T)
    H, L, prefix = np.zeros(B), np.zeros(B), np.zeros((B, T))
    xlogx = lambda p: np.where(p > 0, p * np.log(np.where(p > 0, p, 1.)), 0.)
    E = np.exp(A)
    G = np.where(np.isneginf(A), 0., E * np.where(np.isneginf(A), 0., A))
    for b in range(B):
        for t in range(int(F[b])):
            x = obs[b, t] + (pi if t == 0 else 0.)
            m = x.max()
            e = np.exp(x - m)
            if t == 0:
                a, h = e, np.zeros(S)
            else:
                d = E @ p
                reached = d > 0
                h = np.zeros(S)
                h[reached] = np.log(d[reached]) + ((E @ u)[reached] - (G @ p)[reached]) / d[reached]
                a = e * d
            c = a.sum()
            p = a / c
            u = p * h - xlogx(p)
            prefix[b, t] = u.sum()
            L[b] += math.log(c) + m
        H[b] = prefix[b, F[b] - 1]
    return H, L, prefix


def identity(obs, frames, A, pi):
    """(H, L) float64 through H = L - E[log weight], the expectation taken with forward-backward's posteriors and expected
    transition counts (the float64 route of `state_posteriors` / `expected_counts`), one item per call."""
    obs, A, pi = _f64(obs, A, pi)
    B, T, S = obs.shape
    F = clamp(frames, T)
    H, L = np.zeros(B), np.zeros(B)
    At, pit = torch.from_numpy(A), torch.from_numpy(pi)
    for b in range(B):
        f = int(F[b])
        gamma, Lb, X, _ = posterior._host(torch.from_numpy(obs[b:b + 1]), torch.tensor([f]), At, None, pit, counts=True)
        gamma, X = gamma[0].numpy(), X.numpy()
        expected = 0.
        first = gamma[0] > 0
        expected += (gamma[0][first] * pi[first]).sum()
        for t in range(f):
            on = gamma[t] > 0
            expected += (gamma[t][on] * obs[b, t][on]).sum()
        on = X > 0
        expected += (X[on] * A[on]).sum()
        L[b] = float(Lb[0])
        H[b] = L[b] - expected
    return H, L


def frame_entropies(obs, frames, A, pi):
    """(B,) float64: the sum over an item's frames of the entropies of its per-frame posteriors, an upper bound of H."""
    obs, A, pi = _f64(obs, A, pi)
    gamma = posterior._host(torch.from_numpy(obs), torch.from_numpy(clamp(frames, obs.shape[1])), torch.from_numpy(A), None,
                            torch.from_numpy(pi))[0].numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        return -np.where(gamma > 0, gamma * np.log(gamma), 0.).sum(axis=(1, 2))


# ---- the makers of inputs: float32 arrays, computed once, never written ----
def ragged(B, T, seed):
    """Lengths in 1 .. T; item 0 has T frames and, where there is a second item, the last has 1."""
    frames = np.random.default_rng(seed).integers(1, T + 1, size=B).astype(np.int32)
    frames[0] = T
    if B >= 2:
        frames[B - 1] = 1
    return frames


def left_to_right(S, seed):
    """A log matrix [next, prev] that allows staying and the next two states only, -inf elsewhere; columns normalised."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(S, S, generator=g)
    j, i = torch.meshgrid(torch.arange(S), torch.arange(S), indexing='ij')
    A[(j < i) | (j > i + 2)] = -math.inf
    return torch.log_softmax(A, 0).numpy()


def permutation(S, seed):
    """A log permutation matrix: 0 at [perm[i], i], -inf elsewhere.  Every state has one predecessor: the cancellation
    between log d and (D2 - D3) / d is total, and H stays the entropy of softmax(pi + o_0)."""
    perm = np.random.default_rng(seed).permutation(S)
    A = np.full((S, S), -np.inf, np.float32)
    A[perm, np.arange(S)] = 0.
    return A


@functools.lru_cache(maxsize=None)
def softmax_case(B, T, S, seed, scale=3., matrix='dense'):
    """(obs, frames, A or None, pi): softmax rows of scale <= 3 and a column-normalised matrix of kind `matrix`: 'dense',
    'left_to_right', 'permutation' or None (the uniform model)."""
    assert scale <= 3.
    g = torch.Generator().manual_seed(seed)
    obs = torch.log_softmax(scale * torch.randn(B, T, S, generator=g), 2).numpy()
    pi = torch.log_softmax(torch.randn(S, generator=g), 0).numpy()
    A = {'dense': lambda: torch.log_softmax(scale * torch.randn(S, S, generator=g), 0).numpy(),
         'left_to_right': lambda: left_to_right(S, seed), 'permutation': lambda: permutation(S, seed),
         None: lambda: None}[matrix]()
    return obs, ragged(B, T, seed), A, pi


# (S, T) whose S^T <= 1024 paths are enumerated, each with every kind of matrix
ENUMERATED = [(2, 10), (3, 6), (4, 5), (1, 4)]
ENUMERATED_ITEMS = 3
KINDS = ('dense', 'left_to_right', 'permutation', None)


@functools.lru_cache(maxsize=None)
def enumerated_case(S, T, matrix):
    """(obs, frames, A, pi, enumerate_paths' (H, L, prefix))."""
    obs, frames, A, pi = softmax_case(ENUMERATED_ITEMS, T, S, 10 * S + T, matrix=matrix)
    return obs, frames, A, pi, enumerate_paths(obs, frames, A, pi)


def tensors(*arrays, device='cpu'):
    return [None if a is None else torch.from_numpy(np.array(a)).to(device) for a in arrays]


def numpy(out):
    return tuple(x.detach().cpu().numpy().astype(np.float64) for x in out)


def close(got, want, bound, what=''):
    """|got - want| <= bound elementwise, NaN where and only where `want` has NaN, infinities equal."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN positions differ', got, want)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (what, 'infinities differ')
    ok = np.isfinite(want)
    error = np.abs(got - want)[ok]
    over = error > np.broadcast_to(bound, want.shape)[ok]
    assert not over.any(), (what, f'{int(over.sum())} of {int(ok.sum())} beyond the bound; worst error {error.max():.3e}')
    return float(error.max()) if error.size else 0.


def reference_bound(want):
    return REFERENCE_RTOL * (1. + np.abs(np.asarray(want, np.float64)))


def likelihood_bound(want, frames, T):
    """POSTERIOR.md's bound of a float32 log-likelihood against float64."""
    return RTOL_L * np.abs(np.asarray(want, np.float64)) + ATOL_L_PER_FRAME * clamp(frames, T)


# the two entries as rows of tests/operand_form_cases.py's table (they are not in torbi_amd.__all__, so the table itself has
# no row for them): `forward_entropy` takes its operands where the observation lives, `path_entropy` has a gpu=None route
ENTRIES = [
    ofc.Entry('forward_entropy', [], ofc.OFAP, 'dense',
              lambda o, gpu: entropy.forward_entropy(o[ofc.O], o[ofc.F], o[ofc.A], o[ofc.PI], prefix=True), cpu=True),
    ofc.Entry('path_entropy', [], ofc.OFAP, 'band',
              lambda o, gpu: entropy.path_entropy(o[ofc.O], batch_frames=o[ofc.F], transition=o[ofc.A], initial=o[ofc.PI],
                                                  log_probs=True, gpu=gpu, prefix=True), cpu=True),
]
ENTRY = {e.name: e for e in ENTRIES}


def form_cases(device):
    """(entry name, operand, form) of every non-plain case of the two entries on `device`."""
    return [(e.name, operand, name) for e in ENTRIES for operand in e.operands for name in e.forms(operand, device)
            if name != 'plain']
