"""The tie rules, the growing lists and the -inf order of k-best decoding on an MI355X (csrc/k_best.hpp), bit for bit.

tests/test_k_best_gpu.py draws continuous scores, so no two candidates are ever equal there and every list is full after
one frame.  Here the inputs sit on a quarter-step grid (tests/k_best_cases.py `quantised`: sums are exact, ties are real),
the lists take several frames to fill, and -inf entries force lists whose k-th entry is -inf.  Every comparison is `same`:
indices equal and scores equal as bit patterns, against the brute-force enumerator where it is affordable and against the
host route (which tests/test_k_best_cpu.py holds to that enumerator) elsewhere.  What is asserted about the inputs -- the
share of tied ranks, the presence of -inf paths and of missing ranks -- is asserted on the reference's result alone.

References are computed once per case and shared (`functools.lru_cache`); nothing writes into them."""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import synth
from k_best_cases import brute, same, step_items, quantised, tied_share, model

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def host(obs, frames, trans, init, k):
    t = None if trans is None else torch.as_tensor(trans)
    i, s = torbi_amd.decode_k_best(torch.as_tensor(obs), torch.as_tensor(frames), t, torch.as_tensor(init), k)
    return i.numpy(), s.numpy()


def device(obs, frames, trans, init, k):
    t = None if trans is None else torch.as_tensor(trans).to(DEV)
    i, s = torbi_amd.decode_k_best(torch.as_tensor(obs).to(DEV), torch.as_tensor(frames).to(DEV), t,
                                   torch.as_tensor(init).to(DEV), k)
    assert i.device == DEV and i.dtype == torch.int32 and s.dtype == torch.float32
    return i.cpu().numpy(), s.cpu().numpy()


def ragged(B, T, seed):
    frames = np.clip(synth.lengths(B, 1, T, seed=seed), 1, T).astype(np.int32)
    frames[0] = T
    return frames


def banded(S, tiny):
    return synth.banded_transition(S, max(1.5, S / 16.5), tiny=tiny).astype(np.float32)


def fill_matrix(S):
    return torch.full((S, S), math.log(1. / S), dtype=torch.float32).numpy()


def teeth(want, frames, S, k):
    """What a -inf case must show on the reference to test anything: a path that exists (indices >= 0) with score -inf,
    and a missing rank (-1) exactly where an item has fewer than k paths."""
    idx, sc = want
    assert (np.isneginf(sc) & (idx[:, :, 0] >= 0)).any(), 'no existing path of score -inf in the reference'
    T = idx.shape[2]
    short = [b for b in range(len(frames)) if S ** int(min(max(frames[b], 1), T)) < k]
    assert ((idx[:, :, 0] < 0).any(axis=1) == np.isin(np.arange(len(frames)), short)).all()
    return bool(short)


# ---- a. growing lists: n_t = min(k, S^t) takes several frames to reach k; final selections over short lists ----

GROW = [(2, 32, 8), (2, 5, 5), (3, 16, 5), (3, 7, 4), (5, 32, 4), (6, 32, 4), (33, 32, 3), (1, 4, 6)]


def test_growing_cases_grow():
    """The shapes do what they are there for: lists longer than 1 and shorter than k feed a step, and at (3, 7) the k-th
    candidate falls in the middle of a prev-state's ranks (n_{t-1} does not divide k)."""
    def lengths(S, k, T):
        return [min(k, S ** t) for t in range(T)]
    assert lengths(2, 32, 8)[:6] == [1, 2, 4, 8, 16, 32]
    assert lengths(3, 7, 4) == [1, 3, 7, 7] and 7 % 3 != 0
    for S, k, T in GROW:
        n = lengths(S, k, T)
        assert S == 1 or any(1 < x < k for x in n[:-1]) or (S, k, T) == (33, 32, 3)
    assert 5 * 1 < 32 and 5 * 5 < 32 and 6 * 1 < 32 <= 6 * 6          # final selections over m = S * n < k entries


@functools.lru_cache(maxsize=None)
def grow_case(S, k, T, kind, route):
    B = 5
    seed = 1000 * S + 10 * k + T
    if kind == 'continuous':
        obs, trans, init = model(B, T, S, seed, False)
    else:
        obs, trans, init = quantised(B, T, S, seed, 16, dead=kind == 'dead')
    frames = np.array([T, 1, 2, min(3, T), max(1, T - 1)], dtype=np.int32)
    if route == 'uniform':
        trans = None
    want = brute(obs, frames, fill_matrix(S) if trans is None else trans, init, k)
    return obs, frames, trans, init, want


@pytest.mark.parametrize('S,k,T', GROW)
@pytest.mark.parametrize('kind', ['continuous', 'grid', 'dead'])
@pytest.mark.parametrize('route', ['matrix', 'uniform'])
def test_growing_lists_against_brute_force_and_host(S, k, T, kind, route):
    obs, frames, trans, init, want = grow_case(S, k, T, kind, route)
    got = device(obs, frames, trans, init, k)
    same(got, want)
    same(got, host(obs, frames, trans, init, k))
    # ranks beyond S^F: -inf and -1
    for b, F in enumerate(frames):
        paths = S ** int(F)
        if paths < k:
            assert np.isneginf(got[1][b, paths:]).all() and (got[0][b, paths:] == -1).all()
            assert (got[0][b, :paths] >= 0).all()


# ---- b. ties at the sizes where the kernels branch ----

BRANCH = [(9, 8, 64, 5), (5, 6, 65, 32), (4, 6, 255, 3), (4, 6, 257, 8), (3, 5, 513, 16), (2, 3, 1440, 8), (4, 4, 1440, 3),
          (6, 7, 100, 1)]
# The mixed grid of a (shape, route): the `levels` at which the HOST result has between 0.1 and 0.9 of its adjacent ranks
# tied, with ragged and with full frames (found on the CPU; asserted below on the reference).  k = 1 has no adjacent ranks.
# The band kinds have none: their matrix is the continuous log of a triangle, two paths tie only when they take the same
# multiset of |i - j| steps, and no grid of the observation from 2 to 4096 levels brings the share of every shape inside
# the bounds (most stay below 0.1).  Their mixed run keeps a continuous observation and initial and asserts no share;
# their `all_tied` run still ties candidates inside the lists (prev-states j - d and j + d of equal value).
MIXED = {(9, 8, 64, 5, 'dense'): 64, (5, 6, 65, 32, 'dense'): 256, (4, 6, 255, 3, 'dense'): 64, (4, 6, 257, 8, 'dense'): 64,
         (3, 5, 513, 16, 'dense'): 256, (2, 3, 1440, 8, 'dense'): 256, (4, 4, 1440, 3, 'dense'): 64,
         (6, 7, 100, 1, 'dense'): 256,
         (9, 8, 64, 5, 'uniform'): 1024, (5, 6, 65, 32, 'uniform'): 1024, (4, 6, 255, 3, 'uniform'): 1024,
         (4, 6, 257, 8, 'uniform'): 1024, (3, 5, 513, 16, 'uniform'): 1024, (2, 3, 1440, 8, 'uniform'): 1024,
         (4, 4, 1440, 3, 'uniform'): 4096, (6, 7, 100, 1, 'uniform'): 1024}


@functools.lru_cache(maxsize=None)
def branch_case(B, T, S, k, kind, full, levels):
    """levels = None: the continuous observation and initial of synth.problem."""
    seed = 7 * S + k + B
    if levels is None:
        obs, trans, init = synth.problem(B, T, S, seed=seed)
    else:
        obs, trans, init = quantised(B, T, S, seed, levels)
    if kind.startswith('band'):
        trans = banded(S, kind == 'band_tiny')
    elif kind == 'uniform':
        trans = None
    frames = np.full(B, T, dtype=np.int32) if full else ragged(B, T, S + k)
    return obs, frames, trans, init, host(obs, frames, trans, init, k)


def rank_zero_is_decode(obs, frames, trans, init, got):
    """Rank 0 of a device result against torbi_amd.decode on the same device tensors."""
    want = torbi_amd.decode(torch.as_tensor(obs).to(DEV), torch.as_tensor(frames).to(DEV), torch.as_tensor(trans).to(DEV),
                            torch.as_tensor(init).to(DEV)).cpu().numpy()
    assert np.array_equal(got[0][:, 0], want), np.argwhere(got[0][:, 0] != want)[:10]


@pytest.mark.parametrize('B,T,S,k', BRANCH)
@pytest.mark.parametrize('full', [False, True], ids=['ragged', 'full'])
@pytest.mark.parametrize('kind', ['dense', 'band', 'band_tiny', 'uniform'])
@pytest.mark.parametrize('grid', ['all_tied', 'mixed'])
def test_ties_where_the_kernels_branch(B, T, S, k, full, kind, grid):
    band = kind.startswith('band')
    levels = 16 if grid == 'all_tied' else None if band else MIXED[(B, T, S, k, kind)]
    obs, frames, trans, init, want = branch_case(B, T, S, k, kind, full, levels)
    if k > 1:
        share = tied_share(want[1])
        print(f'tied share of the reference: {share:.3f} at levels = {levels}')
        if not band:
            assert 0.1 <= share <= (1. if grid == 'all_tied' else 0.9), share
    got = device(obs, frames, trans, init, k)
    same(got, want)
    if k == 1:
        rank_zero_is_decode(obs, frames, fill_matrix(S) if trans is None else trans, init, got)


# ---- c. every step instance with several items per workgroup, with ties and with growing lists ----

# (1500 items at k = 4 run two to a workgroup, so that case has no partial last group; 1501 has one)
MULTI = [(4093, 6, 3, 2), (4093, 6, 5, 1), (2047, 5, 3, 4), (1023, 5, 3, 7), (1023, 6, 2, 8), (1500, 5, 64, 4),
         (1501, 5, 64, 4), (3001, 5, 64, 2)]


def test_multi_item_cases_reach_the_instances_they_name():
    assert [step_items(B, S, k) for (B, T, S, k) in MULTI] == [(2, 8), (1, 8), (4, 4), (8, 2), (8, 2), (4, 2), (4, 2), (2, 4)]
    assert all(B % step_items(B, S, k)[1] for (B, T, S, k) in MULTI if B != 1500)


@functools.lru_cache(maxsize=None)
def multi_case(B, T, S, k, kind):
    obs, trans, init = quantised(B, T, S, B + 3 * k, 16, dead=kind == 'dead')
    frames = ragged(B, T, B + k)
    frames[-1] = T
    return obs, frames, trans, init, host(obs, frames, trans, init, k)


@pytest.mark.parametrize('B,T,S,k', MULTI)
@pytest.mark.parametrize('kind', ['grid', 'dead'])
def test_several_items_per_workgroup_with_ties_and_growth(B, T, S, k, kind):
    obs, frames, trans, init, want = multi_case(B, T, S, k, kind)
    assert step_items(B, S, k)[1] > 1 and frames.min() == 1
    same(device(obs, frames, trans, init, k), want)


def test_item_independence_with_ties_and_growth():
    """Items 5 and B - 1 keep their bits when every other item changes: their neighbours in the workgroup (G = 4: items
    4 .. 7, and the tail group), among them an item with a NaN and an item that is -inf everywhere."""
    B, T, S, k = 2047, 6, 3, 4
    assert step_items(B, S, k) == (4, 4)
    obs, trans, init = quantised(B, T, S, 5, 16)
    frames = ragged(B, T, 4)
    keep = [5, B - 1]
    frames[keep] = [T, T - 1]
    a = device(obs, frames, trans, init, k)
    same((a[0][keep], a[1][keep]), brute(obs[keep], frames[keep], trans, init, k))
    other = quantised(B, T, S, 6, 16)[0]
    other[keep] = obs[keep]
    other[4, 2, 1] = np.nan
    other[6] = -np.inf
    other[B - 2] = -np.inf
    frames2 = ragged(B, T, 6)
    frames2[keep] = frames[keep]
    frames2[[4, 6]] = T                  # (so that item 4 reads its NaN)
    b = device(other, frames2, trans, init, k)
    same((b[0][keep], b[1][keep]), (a[0][keep], a[1][keep]))
    assert np.isnan(b[1][4]).all() and (b[0][4] == -1).all()
    assert np.isneginf(b[1][6]).all() and (b[0][6] >= 0).all()          # -inf paths that exist keep their indices
    rest = [4, 6, 7, B - 2]
    want = host(other[rest], frames2[rest], trans, init, k)
    same((b[0][rest], b[1][rest]), want)


# ---- d. -inf is ordered, not skipped ----

@pytest.mark.parametrize('S,k,T', GROW)
@pytest.mark.parametrize('route', ['matrix', 'uniform'])
def test_neg_inf_small_lists(S, k, T, route):
    """The `dead` inputs of (a): the reference holds paths of score -inf that exist and ranks that do not, and the device
    orders the first and blanks the second as the brute-force enumerator does."""
    obs, frames, trans, init, want = grow_case(S, k, T, 'dead', route)
    teeth(want, frames, S, k)
    same(device(obs, frames, trans, init, k), want)


def test_neg_inf_small_cases_have_missing_ranks():
    """(over the whole set: every shape but (33, 32, 3) has an item with fewer than k paths)"""
    for S, k, T in GROW:
        for route in ('matrix', 'uniform'):
            obs, frames, trans, init, want = grow_case(S, k, T, 'dead', route)
            assert teeth(want, frames, S, k) == ((S, k, T) != (33, 32, 3))


@functools.lru_cache(maxsize=None)
def dead_case(B, T, S, k):
    """`quantised(dead=True)` leaves so many finite paths at these sizes that no -inf path reaches the first k ranks, so
    two items are made all -inf: item 1 in its last row (the final selection orders -inf entries by state and rank), item 2
    in row 1 (every later list is k entries of -inf whose pointers are the first k pairs (i, r))."""
    obs, trans, init = quantised(B, T, S, 31 * S + k, 16, dead=True)
    frames = ragged(B, T, S)
    frames[1:3] = T
    obs[1, T - 1] = -np.inf
    obs[2, 1] = -np.inf
    return obs, frames, trans, init, host(obs, frames, trans, init, k)


@pytest.mark.parametrize('B,T,S,k', [(6, 6, 64, 8), (4, 5, 257, 16)])
def test_neg_inf_full_lists(B, T, S, k):
    """S >= k here, so every item has k paths and no rank can be missing: `teeth` asserts that too."""
    obs, frames, trans, init, want = dead_case(B, T, S, k)
    assert not teeth(want, frames, S, k)
    assert np.isneginf(want[1][1:3]).all() and (want[0][1:3] >= 0).all()
    assert (want[0][1, :, T - 1] == 0).all()          # all -inf: state 0's ranks come first
    same(device(obs, frames, trans, init, k), want)


@pytest.mark.parametrize('S,k', [(5, 4), (70, 8), (300, 8)])
def test_state_nothing_enters_keeps_the_first_pairs(S, k):
    """Handmade.  Row 0 of the matrix is -inf: every candidate of state 0 is -inf, so its list of frame 1 is k entries of
    -inf with pointers (0, 0), (1, 0), .. (k - 1, 0), and of frame 2 (0, 0), (0, 1), .. (0, k - 1).  `initial` is finite at
    s0 only, row 1 of the observation at x0 only, row 2 at e1 and e2 only: two finite paths for the item of three frames,
    one for the item of two, and every other result rank is an entry of state 0's list (-inf, the lowest state, ranks in
    order), whose path is [r, 0, 0]."""
    T, s0, x0, e1, e2 = 3, S - 1, 2, 1, 3
    trans = quantised(1, 1, S, S, 16)[1]
    trans[0, :] = -np.inf
    init = np.full(S, -np.inf, dtype=np.float32)
    init[s0] = -0.5
    obs = np.full((2, T, S), -np.inf, dtype=np.float32)
    obs[:, 0] = quantised(2, 1, S, S + 1, 16)[0][:, 0]
    obs[:, 1, x0] = -0.25
    obs[0, 2, e1], obs[0, 2, e2] = -1.0, -0.75
    frames = np.array([3, 2], dtype=np.int32)
    f = np.float32
    head = f(obs[0, 1, x0]) + (f(f(obs[0, 0, s0]) + init[s0]) + trans[x0, s0])
    finite = sorted([(-(f(obs[0, 2, e]) + f(head + trans[e, x0])), e) for e in (e1, e2)])
    idx = np.empty((2, k, T), dtype=np.int32)
    sc = np.full((2, k), -np.inf, dtype=np.float32)
    for q, (v, e) in enumerate(finite):
        idx[0, q], sc[0, q] = [s0, x0, e], -v
    for q in range(2, k):
        idx[0, q] = [q - 2, 0, 0]
    idx[1, 0], sc[1, 0] = [s0, x0, x0], f(obs[1, 1, x0]) + (f(f(obs[1, 0, s0]) + init[s0]) + trans[x0, s0])
    for q in range(1, k):
        idx[1, q] = [q - 1, 0, 0]
    want = (idx, sc)
    same(host(obs, frames, trans, init, k), want)
    if S <= 5:
        same(brute(obs, frames, trans, init, k), want)
    same(device(obs, frames, trans, init, k), want)


# ---- e. rank 0 is the decoder under ties ----

@pytest.mark.parametrize('B,T,S', [(33, 20, 64), (12, 12, 360), (6, 8, 1440)])
@pytest.mark.parametrize('kind', ['dense', 'band', 'band_tiny'])
@pytest.mark.parametrize('k', [1, 4])
def test_rank_zero_is_the_gpu_decode_under_ties(B, T, S, kind, k):
    obs, trans, init = quantised(B, T, S, B + S, 16)
    if kind != 'dense':
        trans = banded(S, kind == 'band_tiny')
    frames = ragged(B, T, 5)
    got = device(obs, frames, trans, init, k)
    rank_zero_is_decode(obs, frames, trans, init, got)
    assert (got[1][:, :-1] >= got[1][:, 1:]).all()


@pytest.mark.parametrize('uniform', [False, True])
def test_rank_zero_is_from_probabilities_under_ties(uniform):
    B, T, S, k = 12, 12, 360, 4
    rng = np.random.default_rng(3)
    p = torch.tensor(rng.integers(1, 5, (B, T, S)) * 0.25, dtype=torch.float32)
    A = None if uniform else torch.tensor(rng.integers(1, 5, (S, S)) * 0.25, dtype=torch.float32)
    pi = torch.tensor(rng.integers(1, 5, S) * 0.25, dtype=torch.float32)
    frames = torch.tensor(ragged(B, T, 9))
    want = torbi_amd.from_probabilities(p, frames, A, pi, gpu=0).cpu()
    i, s = torbi_amd.best_paths(p, k, frames, A, pi, gpu=0)
    assert torch.equal(i[:, 0].cpu().to(want.dtype), want)
    assert tied_share(s.cpu().numpy()) > 0
