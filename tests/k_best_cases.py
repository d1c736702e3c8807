"""What the k-best tests of both routes share: the brute-force enumerator that is the reference of the host route, the exact
comparison, input makers (continuous, small integers, a quarter-step grid with optional -inf entries), the step launch's
choice of instance, and the measure of how many ties a result holds."""
import numpy as np
import torch

import torbi_amd

f32 = np.float32


def brute(obs, frames, trans, init, k):
    """Every path scored in float32 with the contract's order of additions, ranked by the recursive tie rule: at frame t
    the paths into state j are ordered by c = fl(v_{t-1} + A[j, i]) descending, then by i, then by the rank of their
    prefix among the paths into i at t - 1; the result by (value descending, last state, rank)."""
    B, T, S = obs.shape
    indices = np.full((B, k, T), -1, dtype=np.int32)
    scores = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        F = int(min(max(frames[b], 1), T))
        # ranked[j] = [(value, path)] in order
        ranked = [[(f32(obs[b, 0, j]) + f32(init[j]), [j])] for j in range(S)]
        for t in range(1, F):
            new = []
            for j in range(S):
                cands = []
                for i in range(S):
                    for r, (v, path) in enumerate(ranked[i]):
                        c = f32(v) + f32(trans[j, i])
                        cands.append((-c, i, r, c, path))
                cands.sort(key=lambda x: (x[0], x[1], x[2]))
                new.append([(f32(obs[b, t, j]) + c, path + [j]) for (_, _, _, c, path) in cands])
            ranked = new
        final = [(-v, j, r, v, path) for j in range(S) for r, (v, path) in enumerate(ranked[j])]
        final.sort(key=lambda x: (x[0], x[1], x[2]))
        for q, (_, _, _, v, path) in enumerate(final[:k]):
            scores[b, q] = v
            indices[b, q, :F] = path
            indices[b, q, F:] = path[-1]
    return indices, scores


def same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), (got[1], want[1])


def clamp(x):
    """The epsilon round trip best_paths applies to a log observation (torch's CPU ops, as on the host route)."""
    return torbi_amd.viterbi.epsilon_clamp_(torch.tensor(x, dtype=torch.float32)).numpy()


def model(B, T, S, seed, ties):
    rng = np.random.default_rng(seed)
    if ties:        # small integers: ties everywhere
        obs = -rng.integers(0, 3, (B, T, S)).astype(np.float32)
        trans = -rng.integers(0, 3, (S, S)).astype(np.float32)
        init = -rng.integers(0, 2, (S,)).astype(np.float32)
    else:
        obs = rng.standard_normal((B, T, S)).astype(np.float32)
        trans = rng.standard_normal((S, S)).astype(np.float32)
        init = rng.standard_normal(S).astype(np.float32)
    return obs, trans, init


def step_items(B, S, k):
    """(KMAX, G) of the step launch for this shape (torbi_hip.hip kb_step): the rule depends on B, S and k only."""
    kmax = 1
    while kmax < k:
        kmax *= 2
    G = min(8, max(1, 16 // kmax))
    while G > 1 and G * S * 4 > 64 * 1024:
        G //= 2
    jblocks = -(-S // 256)
    while G > 1 and -(-B // G) * jblocks < 512:
        G //= 2
    return kmax, G


def quantised(B, T, S, seed, levels, dead=False):
    """(observation, transition, initial) on the grid -0.25 * {0 .. levels - 1}.  Every sum of a few such values is exact in
    float32, so equal path scores are equal bits on every route and in every order of addition: small `levels` tie almost
    everything, large ones a part.  `dead` puts real -inf in: about 30 % of the matrix entries, one whole matrix row (a state
    nothing can enter), one whole column (a state nothing can leave), about 30 % of `initial` (state 0 stays at 0) and
    about 20 % of the observation entries."""
    rng = np.random.default_rng(seed)
    obs = (-0.25 * rng.integers(0, levels, (B, T, S))).astype(np.float32)
    trans = (-0.25 * rng.integers(0, levels, (S, S))).astype(np.float32)
    init = (-0.25 * rng.integers(0, levels, (S,))).astype(np.float32)
    if dead:
        trans[rng.random((S, S)) < 0.3] = -np.inf
        trans[int(rng.integers(S)), :] = -np.inf
        trans[:, int(rng.integers(S))] = -np.inf
        init[rng.random(S) < 0.3] = -np.inf
        init[0] = 0.
        obs[rng.random((B, T, S)) < 0.2] = -np.inf
    return obs, trans, init


def tied_share(scores):
    """The share of adjacent result ranks, both finite, that hold the same score, over the whole batch."""
    s = np.asarray(scores)
    a, b = s[:, :-1], s[:, 1:]
    both = np.isfinite(a) & np.isfinite(b)
    return float((a[both] == b[both]).mean()) if both.any() else 0.
