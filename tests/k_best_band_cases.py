"""What the tests of the k-best band route share: band matrices over the input makers of k_best_cases, the instance rule of
the forward launch, and a numpy restatement of the route's rule (KBEST.md, "Band route") that also tells, per (item, frame,
state), which path a state took."""
import math

import numpy as np

import k_best_cases as kc

TINY = float(np.log(np.float32(np.finfo(np.float32).tiny)))       # log(tiny), the reference's value outside the pitch band
REACHES = [(2, 2), (0, 0), (0, 3), (3, 0), (5, 2), (31, 31)]
BACKGROUNDS = [-math.inf, TINY, -20.]
MAX_LDS = 159 * 1024

FAST, FALLBACK = 0, 1

# (reach, background, k, levels, with -inf entries): seed 21 of each was looked at on the restatement before it was listed.
# Wide grids (96 and 400 levels: scores down to -24 and -100) bring a state's k-th in-band value down to dmax for a finite
# background; with -inf entries the equal pair is -inf == -inf or, beside a finite background, a finite one.
BOTH = [((2, 2), -20., 4, 96, False), ((5, 2), -20., 8, 96, False), ((31, 31), -20., 8, 96, False),
        ((31, 31), -20., 4, 96, True), ((3, 0), -20., 1, 96, False), ((0, 0), -20., 4, 3, True),
        ((2, 2), -math.inf, 4, 3, True), ((0, 3), -math.inf, 8, 3, True), ((0, 0), -math.inf, 1, 3, True),
        ((5, 2), TINY, 4, 3, True), ((3, 0), TINY, 8, 400, False)]
BOTH_IDS = [f'{r[0]}-{r[1]}-{"inf" if b == -math.inf else int(b)}-k{k}-{"dead" if d else "grid"}' for r, b, k, _, d in BOTH]


def banded(trans, reach_left, reach_right, background):
    """`trans` with `background` everywhere outside the band j - reach_left <= i <= j + reach_right ([next j, prev i])."""
    S = trans.shape[0]
    j, i = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    out = trans.astype(np.float32).copy()
    out[(i < j - reach_left) | (i > j + reach_right)] = np.float32(background)
    return out


def model(B, T, S, seed, reach, background, levels=None, dead=False):
    """(observation, band matrix, initial): continuous scores, or with `levels` the tie grid of k_best_cases.quantised
    (`dead`: with -inf entries), the matrix cut to the band."""
    if levels is None:
        obs, trans, init = kc.model(B, T, S, seed, ties=False)
    else:
        obs, trans, init = kc.quantised(B, T, S, seed, levels, dead=dead)
    return obs, banded(trans, reach[0], reach[1], background), init


def lds_bytes(G, S, k, reach_left, reach_right):
    return 8 * G * k * (S + reach_left + reach_right)


def covered(S, k, reach_left, reach_right, background=-math.inf):
    """torbi_hip_k_best_band_covers's stated rule (B, T >= 1)."""
    return (S % 4 == 0 and 64 <= S <= 3072 and reach_left >= 0 and reach_right >= 0 and reach_left + reach_right + 4 <= 512
            and 1 <= k <= 32 and lds_bytes(1, S, k, reach_left, reach_right) <= MAX_LDS
            and not math.isnan(background) and background != math.inf)


def instance(B, S, k, reach_left, reach_right):
    """(KMAX, G) of kb_band_forward_kernel for a covered call: the rule include/torbi_hip.h states."""
    kmax = 1
    while kmax < k:
        kmax *= 2
    G = min(4, max(1, 16 // kmax))
    while G > 1 and lds_bytes(G, S, k, reach_left, reach_right) > MAX_LDS:
        G //= 2
    while G > 1 and -(-B // G) < 256:
        G //= 2
    return kmax, G


def _first(values, k):
    """The first min(k, count) of `values` (flattened i * n + r) in the order (value descending, index ascending)."""
    order = np.argsort(-values, kind='stable')[:k]
    return values[order], order


def restate(obs, frames, trans, init, k, reach_left, reach_right, background, strict=True):
    """The band route's rule in numpy, float32: per frame dmax = max_i fl(L(i)[0] + background); state j takes the first k of
    its in-band candidates (FAST) where there are k and the k-th is strictly greater than dmax, else the first k over all S
    prev-states with `background` read outside the band (FALLBACK).  Inputs without NaN or +inf.  `strict=False` is the
    WRONG rule, '>=' in place of '>': what a kernel that lets a k-th value equal to dmax pass would compute.

    Returns (indices (B, k, T) int32, scores (B, k) float32, path (B, T - 1, S) int8: FAST, FALLBACK or -1 for a frame the
    item does not have, equal (B, T - 1, S) bool: the in-band list was full and its k-th value EQUAL to dmax)."""
    obs, trans, init = (np.asarray(x, dtype=np.float32) for x in (obs, trans, init))
    B, T, S = obs.shape
    bg = np.float32(background)
    assert not np.isnan(obs).any() and not (obs == np.inf).any() and not np.isnan(trans).any()
    indices = np.full((B, k, T), -1, dtype=np.int32)
    scores = np.full((B, k), -np.inf, dtype=np.float32)
    path = np.full((B, max(T - 1, 0), S), -1, dtype=np.int8)
    equal = np.zeros((B, max(T - 1, 0), S), dtype=bool)
    with np.errstate(invalid='ignore'):
        for b in range(B):
            F = int(min(max(frames[b], 1), T))
            L = (obs[b, 0] + init)[:, None]                               # (S, n)
            ns, pointers = [1], [None]
            for t in range(1, F):
                n = L.shape[1]
                dmax = np.max(L[:, 0] + bg)
                new = np.empty((S, min(k, S * n)), dtype=np.float32)
                ptr = np.empty((S, min(k, S * n)), dtype=np.int64)
                for j in range(S):
                    lo, hi = max(j - reach_left, 0), min(j + reach_right, S - 1)
                    c = (L[lo:hi + 1] + trans[j, lo:hi + 1, None]).reshape(-1)
                    v, order = _first(c, k)
                    full = v.size == k
                    equal[b, t - 1, j] = full and v[-1] == dmax
                    if full and (v[-1] > dmax if strict else v[-1] >= dmax):
                        path[b, t - 1, j] = FAST
                        order = order + lo * n
                    else:
                        path[b, t - 1, j] = FALLBACK
                        a = np.full(S, bg, dtype=np.float32)
                        a[lo:hi + 1] = trans[j, lo:hi + 1]
                        v, order = _first((L + a[:, None]).reshape(-1), k)
                    new[j] = obs[b, t, j] + v
                    ptr[j] = order
                L = new
                ns.append(L.shape[1])
                pointers.append(ptr)
            n = L.shape[1]
            v, order = _first(L.reshape(-1), k)
            scores[b, :v.size] = v
            for q in range(v.size):
                s, r = divmod(int(order[q]), n)
                indices[b, q, F:] = s
                for t in range(F - 1, 0, -1):
                    indices[b, q, t] = s
                    s, r = divmod(int(pointers[t][s, r]), ns[t - 1])
                indices[b, q, 0] = s
    return indices, scores, path, equal


def shares(path):
    """(cells that took the fast path, cells that took the fallback) over the frames that exist."""
    return int((path == FAST).sum()), int((path == FALLBACK).sum())


def both_problem(reach, background, levels, dead):
    """(observation, frames, band matrix, initial) of a BOTH case: 4 items of up to 8 frames at 64 states, seed 21."""
    B, T = 4, 8
    obs, trans, init = model(B, T, 64, 21, reach, background, levels=levels, dead=dead)
    return obs, np.array([T] + [max(1, T - 1 - b) for b in range(B - 1)], dtype=np.int32), trans, init


def tie_left_of_band(k):
    """(observation, frames, band matrix, initial, reach, background) built so that '>' and '>=' against dmax give different
    RESULTS: 64 states, reach (2, 2), background -20 on the quarter-step grid.  Frame 0 holds 0 at states 0 .. 3 and -20
    elsewhere, so dmax = -20; state 40 reads matrix entries 0 over its band 38 .. 42, so its five in-band candidates are -20
    as well: a full list (k <= 4) whose k-th value EQUALS dmax.  The dense order puts the out-of-band candidates of states
    0 .. 3, left of the band and equal, first; an in-band list would point at 38 .. 41.  Frame 1 lifts state 40 by 30, so the
    item's best k paths end there and show the pointers."""
    assert 1 <= k <= 4
    reach, background = (2, 2), -20.
    obs, trans, init = model(2, 3, 64, 3, reach, background, levels=8)
    init[:] = 0.
    obs[:, 0, :] = -20.
    obs[:, 0, :4] = 0.
    trans[40, 38:43] = 0.
    obs[:, 1, 40] = 30.
    return obs, np.array([2, 3], dtype=np.int32), trans, init, reach, background
