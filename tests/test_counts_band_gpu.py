"""The band route of the expected counts on an MI355X (csrc/counts_band.hpp, torbi_amd.forward_backward_counts_banded and the
routing of torbi_amd.expected_counts / log_likelihood) against the float64 host route on the FULL matrix, gathered along the
band's diagonals.

The bounds are those of tests/test_counts_gpu.py::check_counts, applied to the in-band entries.  A workgroup owns G whole
items per tile, G = 8 halved while rows and plane do not fit the LDS and while there are fewer workgroups than compute
units: batches below 512 items run G = 1, so the shapes with 515 to 4100 items are here for G = 2 and 8, a partial last tile
and (4100 items: 513 tiles for 512 workgroups) the persistent loop over tiles.
"""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import inputs, posterior, synth, training

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
TINY = float(np.log(np.finfo(np.float32).tiny))
NINF = -math.inf


def ragged(B, T, seed):
    """Ragged lengths with frames[0] = T; 1, 2 and out-of-range values (clamped to [1, T]) where the batch has room."""
    frames = synth.lengths(B, -3, T + 5, seed=seed).astype(np.int32)
    for b, f in enumerate((T, 1, 2, T + 9, -2)):
        if b < B:
            frames[b] = f
    return frames


def peaked(B, T, S, half_width, seed):
    """Posteriorgram rows peaked around a pitch track that moves inside the band (log of a normalised row)."""
    rng = np.random.default_rng(seed)
    x = np.arange(S)
    obs = np.empty((B, T, S), dtype=np.float32)
    for b in range(B):
        c = rng.integers(S // 4, 3 * S // 4)
        for t in range(T):
            c = int(np.clip(c + rng.integers(-half_width + 1, half_width), 0, S - 1))
            row = np.exp(-0.5 * ((x - c) / 3.) ** 2) + 1e-3 * rng.random(S)
            obs[b, t] = np.log(row / row.sum())
    return obs


def band_matrix(S, reach_left, reach_right, background, seed):
    """Random band entries (not Toeplitz), `background` everywhere else; [next j, prev i] with j - left <= i <= j + right."""
    trans = synth.scores(synth.STREAM_TRANSITION, (S, S), seed)
    j, i = np.arange(S)[:, None], np.arange(S)[None, :]
    inside = (i >= j - reach_left) & (i <= j + reach_right)
    return np.where(inside, trans, np.float32(background)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(B, T, S, reach_left, reach_right, background):
    """(observation, frames, transition, initial) of one case, read-only.  The 1440-state cases are the pitch matrices with
    peaked rows, the others random."""
    if S == 1440:
        obs = peaked(B, T, S, 12, seed=1)
        trans = synth.banded_transition(S, 12, tiny=background != NINF)
        init = np.log(np.full(S, 1. / S, dtype=np.float32))
    else:
        seed = B + T + S
        obs = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), seed)
        init = synth.scores(synth.STREAM_INITIAL, (S,), seed)
        trans = band_matrix(S, reach_left, reach_right, background, seed)
    out = (obs, ragged(B, T, seed=S), trans, init)
    for a in out:
        a.setflags(write=False)
    return out


def gather(X, reach_left, reach_right):
    """The diagonals of an (S, S) numpy matrix [next, prev] in the layout of band_counts: out[k, j] = X[j, j - left + k]
    (the reaches clamped to S - 1), 0 where the matrix clips the diagonal."""
    S = X.shape[0]
    left, right = min(reach_left, S - 1), min(reach_right, S - 1)
    out = np.zeros((left + right + 1, S), dtype=X.dtype)
    for k in range(left + right + 1):
        j = np.arange(max(0, left - k), min(S, S + left - k))
        out[k, j] = X[j, j - left + k]
    return out


def host(obs, frames, trans, init, reach_left, reach_right, weights=None):
    """training._host_counts in float64 on the full matrix: (band counts, initial counts, L)."""
    _, L, X, I = training._host_counts(torch.from_numpy(np.array(obs)), torch.from_numpy(np.array(frames)),
                                       torch.from_numpy(np.array(trans)), torch.from_numpy(np.array(init)),
                                       None if weights is None else torch.as_tensor(weights))
    return gather(X.numpy(), reach_left, reach_right), I.numpy(), L.numpy()


@functools.lru_cache(maxsize=None)
def reference(*case):
    """`host` on `problem(*case)`, computed once."""
    return host(*problem(*case), case[3], case[4])


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def device(obs, frames, trans, init, reach_left, reach_right, background, weights=None, workspace=None):
    w = None if weights is None else torch.as_tensor(weights, dtype=torch.float32).to(DEV)
    out = torbi_amd.forward_backward_counts_banded(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), reach_left,
                                                   reach_right, background, item_weights=w, workspace=workspace)
    S = obs.shape[2]
    W = min(reach_left, S - 1) + min(reach_right, S - 1) + 1
    assert all(x.device == DEV and x.dtype == torch.float32 for x in out)
    assert out[2].shape == (W, S) and out[3].shape == (S,)
    return out


def check_counts(X, I, rX, rI, frames, T, what=''):
    """tests/test_counts_gpu.py::check_counts on the in-band entries, printing every figure before it asserts (share of the
    bound in brackets)."""
    X, I = X.cpu().numpy().astype(np.float64), I.cpu().numpy().astype(np.float64)
    F = np.clip(np.asarray(frames), 1, T)
    dX, dI = np.abs(X - rX), np.abs(I - rI)
    bX, bI = 1e-4 * np.abs(rX) + 1e-6 * np.abs(rX).max(), 1e-4 * np.abs(rI) + 1e-6 * np.abs(rI).max()
    pairs = max((F - 1).sum(), 1)
    share = lambda d, b: float(np.max(np.where(d > 0, d / np.maximum(b, 1e-300), 0.)))
    print(f'{what} X elementwise {dX.max():.2e} ({share(dX, bX):.4f}) sum {dX.sum():.2e} ({dX.sum() / (1e-5 * pairs):.4f}) '
          f'I elementwise {dI.max():.2e} ({share(dI, bI):.4f}) sum {dI.sum():.2e} ({dI.sum() / (1e-5 * len(F)):.4f})')
    assert np.all(dX <= bX), dX.max()
    assert dX.sum() <= 1e-5 * pairs, (dX.sum(), pairs)
    assert np.all(dI <= bI), dI.max()
    assert dI.sum() <= 1e-5 * len(F), dI.sum()


CASES = [(1, 1, 8, 1, 1, NINF),                    # no pairs: X = 0
         (3, 40, 64, 2, 5, NINF),                  # asymmetric reach: a transposed or mirrored diagonal
         (3, 40, 64, 5, 2, -20.0),                 # ... the reaches swapped, a finite background
         (17, 33, 65, 0, 0, NINF),                 # diagonal only
         (9, 12, 37, 36, 36, -3.0),                # a band wider than the matrix, clipped on both edges
         (5, 30, 1441, 12, 12, NINF),              # two states per thread, unaligned rows
         (8, 60, 1440, 11, 11, NINF),              # the pitch matrix, -inf outside
         (8, 60, 1440, 11, 11, TINY),              # ... log(tiny) outside
         (4, 10, 4096, 3, 3, NINF),                # plane and rows: 147 KB of LDS
         (515, 4, 65, 2, 1, -6.0),                 # G = 2, partial last tile
         (1030, 3, 37, 1, 2, NINF),                # G = 4 on 256 compute units, partial last tile
         (2050, 3, 33, 0, 3, NINF),                # G = 8
         (4100, 3, 33, 1, 2, NINF)]                # G = 8, 513 tiles for 512 workgroups: the persistent loop


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_shapes_against_float64(case):
    B, T, S, left, right, background = case
    obs, frames, trans, init = problem(*case)
    post, L, X, I = device(obs, frames, trans, init, left, right, background)
    rX, rI, rL = reference(*case)
    assert np.isfinite(rL).all()
    if T == 1:
        assert not X.any()
    check_counts(X, I, rX, rI, frames, T, 'x'.join(str(v) for v in case))
    # clipped positions are exactly 0
    clipped = gather(np.ones((S, S)), left, right) == 0
    assert not X.cpu().numpy()[clipped].any()
    # posterior and log-likelihood are those of forward_backward_banded, bit for bit
    post2, L2 = torbi_amd.forward_backward_banded(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), left, right,
                                                  background)
    assert torch.equal(post, post2) and torch.equal(L, L2)


def test_a_plane_that_does_not_fit():
    B, T, S = 2, 4, 4096
    obs, frames, trans, init = (to_dev(x) for x in problem(B, T, S, 31, 32, NINF))
    assert not posterior._counts_covered(B, T, S, 31, 32, NINF) and posterior._covered(B, T, S, 31, 32, NINF)
    with pytest.raises(RuntimeError, match='does not cover'):
        torbi_amd.forward_backward_counts_banded(obs, frames, trans, init, 31, 32)
    with pytest.raises(RuntimeError, match='>= 0'):
        torbi_amd.forward_backward_counts_banded(obs, frames, trans, init, -1, 32)
    # The routing cannot be shown at 4096 states: `viterbi.band_over` finds bands up to 3072 states only, so auto would go
    # dense there whatever the plane needs.  Instead: a band `state_posteriors` sends to its band kernel and that is too
    # wide for the plane, 27 diagonals of 1440 states
    B, T, S = 2, 4, 1440
    obs = to_dev(synth.scores(synth.STREAM_OBSERVATION, (B, T, S), 3))
    init = to_dev(synth.scores(synth.STREAM_INITIAL, (S,), 3))
    trans = to_dev(band_matrix(S, 13, 13, NINF, 3))
    assert torbi_amd.posterior_route(trans, B, T, S, gpu=0, log_probs=True) == 'band'
    assert torbi_amd.counts_route(trans, B, T, S, gpu=0, log_probs=True) == 'dense'
    auto = torbi_amd.expected_counts(obs, None, trans, init, log_probs=True, gpu=0)
    dense = torbi_amd.expected_counts(obs, None, trans, init, log_probs=True, gpu=0, route='dense')
    assert all(torch.equal(a, b) for a, b in zip(auto, dense))
    with pytest.raises(RuntimeError, match='band'):
        torbi_amd.expected_counts(obs, None, trans, init, log_probs=True, gpu=0, route='band')
    with pytest.raises(RuntimeError, match='band'):
        torbi_amd.log_likelihood(obs, None, trans, init, route='band')


def test_weights_are_linear_and_skip_items():
    case = (515, 4, 65, 2, 1, -6.0)                 # G = 2: item 3 (NaN) shares its tile with item 2, item 5 (weight 0) with 4
    B, T, S, left, right, background = case
    obs, frames, trans, init = problem(*case)
    frames = np.array(frames)
    frames[2:6] = T                                 # (the NaN below has to be inside its item's frames)
    bad = np.array(obs)
    bad[3, 2, 7] = math.nan                         # L_3 = NaN
    g = np.random.default_rng(4).uniform(0.5, 1.5, size=B).astype(np.float32)
    g[5] = 0.
    post, L, X, I = device(bad, frames, trans, init, left, right, background, g)
    assert math.isnan(L[3].item()) and torch.isnan(post[3]).all() and torch.isfinite(L[2]) and torch.isfinite(post[2]).all()
    # against float64 with the same weights and item 3 left out.  X and I are linear in the weights, so their bounds are
    # check_counts' with every item's share of the two totals scaled by its weight
    live = g.astype(np.float64)
    live[3] = 0.
    rX, rI, _ = host(obs, frames, trans, init, left, right, live)
    Xn, In = X.cpu().numpy().astype(np.float64), I.cpu().numpy().astype(np.float64)
    dX, dI = np.abs(Xn - rX), np.abs(In - rI)
    print(f'weighted: X {dX.max():.2e} sum {dX.sum():.2e} of {1e-5 * (live * (frames - 1)).sum():.2e}; I {dI.max():.2e} sum '
          f'{dI.sum():.2e} of {1e-5 * live.sum():.2e}')
    assert np.all(dX <= 1e-4 * np.abs(rX) + 1e-6 * np.abs(rX).max()), dX.max()
    assert dX.sum() <= 1e-5 * (live * (frames - 1)).sum()
    assert np.all(dI <= 1e-4 * np.abs(rI) + 1e-6 * np.abs(rI).max()), dI.max()
    assert dI.sum() <= 1e-5 * live.sum()
    # the NaN item: finite counts, the same bits as with its data clean and its weight 0, or its NaN data and its weight 0
    g0 = g.copy()
    g0[3] = 0.
    X0, I0 = device(obs, frames, trans, init, left, right, background, g0)[2:]
    assert torch.isfinite(X).all() and torch.isfinite(I).all() and torch.equal(X, X0) and torch.equal(I, I0)
    X1, I1 = device(bad, frames, trans, init, left, right, background, g0)[2:]
    assert torch.equal(X, X1) and torch.equal(I, I1)
    # twice the weights, mixed signs, unit weights against None
    X2, I2 = device(bad, frames, trans, init, left, right, background, 2 * g)[2:]
    assert torch.allclose(X2, 2 * X, rtol=1e-6, atol=1e-7 * X.abs().max().item())
    assert torch.allclose(I2, 2 * I, rtol=1e-6, atol=1e-7 * I.abs().max().item())
    Xm = device(bad, frames, trans, init, left, right, background, -g)[2]
    assert torch.equal(Xm, -X)
    ones = device(obs, frames, trans, init, left, right, background, np.ones(B, dtype=np.float32))
    none = device(obs, frames, trans, init, left, right, background)
    assert torch.equal(ones[2], none[2]) and torch.equal(ones[3], none[3])
    # posterior and L do not depend on the weights
    post3, L3 = torbi_amd.forward_backward_banded(to_dev(bad), to_dev(frames), to_dev(trans), to_dev(init), left, right,
                                                  background)
    assert torch.equal(post.nan_to_num(), post3.nan_to_num()) and torch.equal(L.nan_to_num(), L3.nan_to_num())


def test_broken_promise_is_loud():
    case = (3, 40, 64, 2, 2, NINF)
    obs, frames, trans, init = problem(*case)
    trans = trans.copy()
    trans[20, 23] = -1.5                            # just outside the stated band: i = j + reach_right + 1
    post, L, X, I = device(obs, frames, trans, init, 2, 2, NINF)
    F = np.clip(frames, 1, 40)
    valid = torch.from_numpy(np.arange(40)[None, :] < F[:, None]).to(DEV)
    assert torch.isnan(L).all() and torch.isnan(post[valid]).all() and (post[~valid] == 0).all()
    assert torch.isnan(X).all() and torch.isnan(I).all()
    post, L, X, I = device(obs, frames, trans, init, 2, 3, NINF)
    rX, rI, _ = host(obs, frames, trans, init, 2, 3)
    check_counts(X, I, rX, rI, frames, 40, 'the band stated wide enough')


def test_identical_calls_give_identical_bits():
    case = (515, 4, 65, 2, 1, -6.0)
    g = np.linspace(0.5, 1.5, case[0]).astype(np.float32)
    a = device(*problem(*case), *case[3:], g)
    b = device(*problem(*case), *case[3:], g)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    case = (8, 60, 1440, 11, 11, NINF)
    a = device(*problem(*case), *case[3:])
    b = device(*problem(*case), *case[3:])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_graph_capture_replays_on_new_observations_and_weights():
    B, T, S = 20, 25, 400
    obs = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), 13)
    obs2 = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), 14)
    init = synth.scores(synth.STREAM_INITIAL, (S,), 13)
    trans = band_matrix(S, 6, 3, -40.0, 13)
    frames = np.clip(synth.lengths(B, 1, T, seed=5), 1, T).astype(np.int32)
    tobs, tframes, ttrans, tinit = (torch.as_tensor(np.ascontiguousarray(x)).to(DEV) for x in (obs, frames, trans, init))
    g = torch.linspace(0.5, 2., B, device=DEV)
    g2 = torch.linspace(-1., 1., B, device=DEV)
    ws = torch.empty(torbi_amd.expected_counts_banded_workspace_bytes(B, T, S, 6, 3), dtype=torch.uint8, device=DEV)
    run = lambda o, w: torbi_amd.forward_backward_counts_banded(o, tframes, ttrans, tinit, 6, 3, -40.0, item_weights=w,
                                                                workspace=ws)
    eager = [x.clone() for x in run(tobs, g)]
    eager2 = [x.clone() for x in run(torch.as_tensor(obs2).to(DEV), g2)]
    assert not torch.equal(eager[2], eager2[2])
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = run(tobs, g)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    tobs.copy_(torch.as_tensor(obs2))
    g.copy_(g2)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager2))


ROUTED = (24, 40, 320, 4, 4, NINF)                 # a band `viterbi.band_over` accepts: S % 4 == 0, 64 <= S


def test_expected_counts_takes_the_band_route():
    B, T, S, left, right, _ = ROUTED
    obs, frames, trans, init = (torch.from_numpy(np.array(x)) for x in problem(*ROUTED))
    assert torbi_amd.counts_route(trans, B, T, S, gpu=0, log_probs=True) == 'band'
    assert torbi_amd.counts_route(trans, B, T, S, gpu=None, log_probs=True) == 'dense'
    dense_matrix = torch.from_numpy(synth.problem(1, 1, S, seed=3)[1])
    assert torbi_amd.counts_route(dense_matrix, B, T, S, gpu=0, log_probs=True) == 'dense'
    prepared, _, init_d = inputs.model(trans, init, True, S, DEV)
    obs_d = inputs.observation(obs, True, DEV)
    X, I, L = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0)
    _, L2, Xb, I2 = torbi_amd.forward_backward_counts_banded(obs_d, frames, prepared, init_d, left, right)
    assert X.shape == (S, S) and torch.equal(X, torbi_amd.band_counts_to_dense(Xb, left, right))
    assert torch.equal(I, I2) and torch.equal(L, L2)
    named = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0, route='band')
    assert all(torch.equal(a, b) for a, b in zip(named, (X, I, L)))
    # exactly zero outside the band; both routes within the bounds of the float64 route
    j, i = np.arange(S)[:, None], np.arange(S)[None, :]
    inside = torch.from_numpy((i >= j - left) & (i <= j + right)).to(DEV)
    assert not X[~inside].any()
    dX, dI, dL = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0, route='dense')
    plain = torbi_amd.forward_backward_counts(obs_d, frames, prepared, init_d)
    assert torch.equal(dX, plain[2]) and torch.equal(dI, plain[3]) and torch.equal(dL, plain[1])
    rX, rI, _ = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=None)
    rX, rI = rX.numpy().astype(np.float64), rI.numpy().astype(np.float64)
    check_counts(X, I, rX, rI, frames.numpy(), T, 'expected_counts, band')
    check_counts(dX, dI, rX, rI, frames.numpy(), T, 'expected_counts, dense')


def test_log_likelihood_gradients_match_the_float64_route():
    """The bounds of tests/test_counts_gpu.py::test_log_likelihood_gradients_match_the_float64_route, on the band."""
    B, T, S, left, right, _ = ROUTED
    obs, frames, trans, init = problem(*ROUTED)
    w = torch.as_tensor(np.random.default_rng(2).uniform(0.5, 1.5, B))
    leaves = {}
    for where in ('cpu', 'gpu', 'dense'):
        args = [torch.as_tensor(np.array(x)) for x in (obs, trans, init)]
        args = [a.double() for a in args] if where == 'cpu' else [a.to(DEV) for a in args]
        args = [a.requires_grad_() for a in args]
        fr = torch.as_tensor(np.array(frames)).to(args[0].device)
        L = torbi_amd.log_likelihood(args[0], fr, args[1], args[2], route='dense' if where == 'dense' else 'auto')
        (L * w.to(L.device, L.dtype)).sum().backward()
        leaves[where] = [L.detach().cpu().double()] + [a.grad.cpu().double().numpy() for a in args]
    c, g, d = leaves['cpu'], leaves['gpu'], leaves['dense']
    F = np.clip(frames, 1, T)
    # the forward took the band route: its L, not the dense route's
    banded = torbi_amd.forward_backward_banded(to_dev(obs), to_dev(frames), to_dev(trans), to_dev(init), left, right)[1]
    assert torch.equal(g[0], banded.cpu().double())
    assert np.all(np.abs(g[0].numpy() - c[0].numpy()) <= 1e-6 * np.abs(c[0].numpy()) + 4e-6 * F)
    assert np.abs(g[1] - c[1]).max() <= 1e-4
    j, i = np.arange(S)[:, None], np.arange(S)[None, :]
    inside = (i >= j - left) & (i <= j + right)
    assert not g[2][~inside].any() and not c[2][~inside].any()
    check_counts(torch.as_tensor(g[2]), torch.as_tensor(g[3]), c[2], c[3], F, T, 'gradients, band')
    check_counts(torch.as_tensor(d[2]), torch.as_tensor(d[3]), c[2], c[3], F, T, 'gradients, dense')


def test_baum_welch_on_the_band():
    """Three EM steps on transition and initial: the total L does not decrease, the matrix keeps its -inf outside the band
    and every step takes the band route."""
    B, T, S, left, right, _ = ROUTED
    obs, frames, trans, init = (to_dev(x) for x in problem(*ROUTED))
    j, i = np.arange(S)[:, None], np.arange(S)[None, :]
    inside = torch.from_numpy((i >= j - left) & (i <= j + right)).to(DEV)
    # a proper model: columns (next states of one previous state) and the initial distribution sum to 1
    trans = trans - torch.logsumexp(trans, dim=0, keepdim=True)
    init = init - torch.logsumexp(init, dim=0)
    totals = []
    for _ in range(3):
        assert torbi_amd.counts_route(trans, B, T, S, gpu=0, log_probs=True) == 'band'
        X, I, L = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0)
        totals.append(float(L.double().sum()))
        trans = torch.log(X / X.sum(dim=0, keepdim=True))
        init = torch.log(I / I.sum())
        assert (trans[~inside] == NINF).all()
    L = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0)[2]
    totals.append(float(L.double().sum()))
    assert all(b >= a - 1e-6 * abs(a) for a, b in zip(totals, totals[1:])), totals
    assert totals[-1] > totals[0]
