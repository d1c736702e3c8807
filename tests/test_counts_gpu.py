"""torbi_amd.forward_backward_counts / expected_counts / log_likelihood on an MI355X (csrc/counts.hpp) against the float64
host route, which tests/test_counts_cpu.py checks against brute force and plain autograd."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import synth, training

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def to_dev(*xs):
    return [torch.as_tensor(np.ascontiguousarray(x)).to(DEV) for x in xs]


def host(obs, frames, trans, init, weights=None):
    _, L, X, I = training._host_counts(torch.as_tensor(obs), torch.as_tensor(frames), torch.as_tensor(trans),
                                       torch.as_tensor(init), None if weights is None else torch.as_tensor(weights))
    return X.numpy(), I.numpy(), L.numpy()


def device(obs, frames, trans, init, weights=None):
    args = to_dev(obs, frames, trans, init)
    w = None if weights is None else torch.as_tensor(weights, dtype=torch.float32).to(DEV)
    post, L, X, I = torbi_amd.forward_backward_counts(*args, item_weights=w)
    assert X.dtype == I.dtype == torch.float32 and X.shape == (obs.shape[2],) * 2
    return post, L, X, I


def check_counts(X, I, rX, rI, frames, T):
    X, I = X.cpu().numpy().astype(np.float64), I.cpu().numpy().astype(np.float64)
    F = np.clip(np.asarray(frames), 1, T)
    dX, dI = np.abs(X - rX), np.abs(I - rI)
    assert np.all(dX <= 1e-4 * np.abs(rX) + 1e-6 * np.abs(rX).max()), dX.max()
    assert dX.sum() <= 1e-5 * max((F - 1).sum(), 1), (dX.sum(), (F - 1).sum())
    assert np.all(dI <= 1e-4 * np.abs(rI) + 1e-6 * np.abs(rI).max()), dI.max()
    assert dI.sum() <= 1e-5 * len(F), dI.sum()


SHAPES = [(1, 1, 3), (1, 500, 1440), (3, 50, 200), (17, 64, 65), (64, 100, 256), (512, 40, 1440), (4, 20, 4096),
          (5, 30, 1441), (9, 12, 37), (520, 8, 1441), (700, 6, 999),
          (2, 4, 5), (3, 5, 8), (4, 3, 31)]           # few items, few states: the direct step with KS = 1 (below 16 states), 2


@pytest.mark.parametrize('B,T,S', SHAPES)
def test_dense_shapes_against_float64(B, T, S):
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S)
    frames = np.clip(synth.lengths(B, 1, T, seed=S), 1, T).astype(np.int32)
    frames[0] = T
    post, L, X, I = device(obs, frames, trans, init)
    rX, rI, _ = host(obs, frames, trans, init)
    check_counts(X, I, rX, rI, frames, T)
    # posterior and log-likelihood are those of forward_backward, bit for bit
    post2, L2 = torbi_amd.forward_backward(*to_dev(obs, frames, trans, init))
    assert torch.equal(post, post2) and torch.equal(L, L2)


def test_weights_are_linear_and_skip_items():
    B, T, S = 40, 30, 300
    obs, trans, init = synth.problem(B, T, S, seed=21)
    frames = np.clip(synth.lengths(B, 1, T, seed=2), 1, T).astype(np.int32)
    obs = obs.copy()
    obs[3, 5, 7] = math.nan                                         # L_3 = NaN
    rng = np.random.default_rng(4)
    g = rng.uniform(-1, 2, size=B).astype(np.float32)
    g[5] = 0.
    post, L, X, I = device(obs, frames, trans, init, g)
    assert math.isnan(L[3].item())
    # the weighted sum of per-item host counts
    rX, rI = 0., 0.
    for b in range(B):
        if b == 3 or g[b] == 0:
            continue
        x, i, _ = host(obs[b:b + 1], frames[b:b + 1], trans, init)
        rX, rI = rX + float(g[b]) * x, rI + float(g[b]) * i
    Xn, In = X.cpu().numpy().astype(np.float64), I.cpu().numpy().astype(np.float64)
    scale = np.abs(rX).max()
    assert np.all(np.abs(Xn - rX) <= 1e-4 * np.abs(rX) + 1e-5 * scale), np.abs(Xn - rX).max()
    assert np.all(np.abs(In - rI) <= 1e-4 * np.abs(rI) + 1e-5 * np.abs(rI).max())
    # zero weight on the NaN item and on item 5: the same bits as without those items' weights
    g0 = g.copy()
    g0[3] = 0.
    X0 = device(obs, frames, trans, init, g0)[2]
    assert torch.isfinite(X).all() and torch.equal(X, X0)
    # linear in the weights
    X2 = device(obs, frames, trans, init, 2 * g)[2]
    assert torch.allclose(X2, 2 * X, rtol=1e-6, atol=1e-7 * X.abs().max().item())
    # posterior and L do not depend on the weights
    post3, L3 = torbi_amd.forward_backward(*to_dev(obs, frames, trans, init))
    assert torch.equal(post.nan_to_num(), post3.nan_to_num()) and torch.equal(L.nan_to_num(), L3.nan_to_num())


def test_identical_calls_give_identical_bits():
    B, T, S = 70, 30, 1440
    obs, trans, init = synth.problem(B, T, S, seed=12)
    frames = np.clip(synth.lengths(B, 1, T, seed=3), 1, T).astype(np.int32)
    g = np.linspace(0.5, 1.5, B).astype(np.float32)
    a = device(obs, frames, trans, init, g)
    b = device(obs, frames, trans, init, g)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_graph_capture_replays_on_new_observations_and_weights():
    B, T, S = 20, 25, 400
    obs, trans, init = synth.problem(B, T, S, seed=13)
    obs2 = synth.problem(B, T, S, seed=14)[0]
    frames = np.clip(synth.lengths(B, 1, T, seed=5), 1, T).astype(np.int32)
    tobs, tframes, ttrans, tinit = to_dev(obs, frames, trans, init)
    g = torch.linspace(0.5, 2., B, device=DEV)
    g2 = torch.linspace(-1., 1., B, device=DEV)
    ws = torch.empty(torbi_amd.expected_counts_workspace_bytes(B, T, S), dtype=torch.uint8, device=DEV)
    run = lambda o, w: torbi_amd.forward_backward_counts(o, tframes, ttrans, tinit, item_weights=w, workspace=ws)
    eager = [x.clone() for x in run(tobs, g)]
    eager2 = [x.clone() for x in run(torch.as_tensor(obs2).to(DEV), g2)]
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


def test_log_likelihood_gradients_match_the_float64_route():
    B, T, S = 24, 40, 300
    obs, trans, init = synth.problem(B, T, S, seed=31)
    frames = np.clip(synth.lengths(B, 1, T, seed=6), 1, T).astype(np.int32)
    w = torch.as_tensor(np.random.default_rng(2).uniform(0.5, 1.5, B))
    leaves = {}
    for where in ('cpu', 'gpu'):
        args = [torch.as_tensor(np.ascontiguousarray(x)) for x in (obs, trans, init)]
        if where == 'gpu':
            args = [a.to(DEV) for a in args]
        else:
            args = [a.double() for a in args]
        args = [a.requires_grad_() for a in args]
        fr = torch.as_tensor(frames).to(args[0].device)
        L = torbi_amd.log_likelihood(args[0], fr, args[1], args[2])
        (L * w.to(L.device, L.dtype)).sum().backward()
        leaves[where] = [L.detach().cpu().double()] + [a.grad.cpu().double().numpy() for a in args]
    c, g = leaves['cpu'], leaves['gpu']
    F = np.clip(frames, 1, T)
    assert np.abs(g[1] - c[1]).max() <= 1e-4
    check_counts(torch.as_tensor(g[2]), torch.as_tensor(g[3]), c[2], c[3], F, T)


def test_baum_welch_on_the_device():
    """Five EM steps on transition and initial (emissions fixed) at 64 x 200 x 256: the total L does not decrease."""
    B, T, S = 64, 200, 256
    rng = np.random.default_rng(8)
    A = np.full((S, S), 0.2 / (S - 1)) + np.eye(S) * (0.8 - 0.2 / (S - 1))   # [next, prev], columns sum to 1
    states = np.zeros((B, T), dtype=np.int64)
    states[:, 0] = rng.integers(0, S, size=B)
    for t in range(1, T):
        cum = np.cumsum(A[:, states[:, t - 1]], axis=0)                     # (S, B)
        states[:, t] = np.minimum((cum < rng.uniform(size=B)[None, :]).sum(axis=0), S - 1)
    means = np.arange(S) * 0.5
    y = means[states] + rng.standard_normal((B, T))
    obs = torch.as_tensor((-0.5 * (y[..., None] - means) ** 2).astype(np.float32)).to(DEV)
    frames = torch.as_tensor(np.clip(synth.lengths(B, 1, T, seed=9), 1, T).astype(np.int32)).to(DEV)
    trans = torch.log(torch.as_tensor(rng.dirichlet(np.ones(S), size=S).T.astype(np.float32))).to(DEV)
    init = torch.full((S,), -math.log(S), device=DEV)
    totals = []
    for _ in range(5):
        X, I, L = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0)
        totals.append(float(L.double().sum()))
        trans = torch.log(X / X.sum(dim=0, keepdim=True))
        init = torch.log(I / I.sum())
    assert all(b >= a - 1e-6 * abs(a) for a, b in zip(totals, totals[1:])), totals
    assert totals[-1] > totals[0]
