"""torbi_amd.expected_counts / log_likelihood on the host (float64 route) against brute-force path enumeration, plain torch
autograd and the Baum-Welch property, and the C-ABI surface of torbi_hip_forward_backward_counts without a device."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, synth, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clamp(x):
    """from_probabilities' epsilon round trip on log inputs."""
    t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).clone()
    torch.exp_(t)
    t += torch.finfo(torch.float32).tiny
    torch.log_(t)
    return t.numpy()


def brute(obs, frames, trans, init, weights):
    """Counts by enumerating all S^F paths of every item, float64: (X (S, S) [next, prev], I (S,), L (B,))."""
    obs, trans, init = (np.asarray(x, dtype=np.float64) for x in (obs, trans, init))
    B, T, S = obs.shape
    X, I, L = np.zeros((S, S)), np.zeros(S), np.zeros(B)
    for b in range(B):
        F = int(np.clip(frames[b], 1, T))
        paths = list(itertools.product(range(S), repeat=F))
        lp = np.array([init[p[0]] + obs[b, 0, p[0]] + sum(trans[p[t], p[t - 1]] + obs[b, t, p[t]] for t in range(1, F))
                       for p in paths])
        L[b] = np.logaddexp.reduce(lp)
        prob = np.exp(lp - L[b])
        for p, q in zip(paths, prob):
            I[p[0]] += weights[b] * q
            for t in range(1, F):
                X[p[t], p[t - 1]] += weights[b] * q
    return X, I, L


def problem(B, T, S, seed):
    rng = np.random.default_rng(seed)
    obs = np.log(rng.dirichlet(np.ones(S), size=(B, T))).astype(np.float32)
    trans = np.log(rng.dirichlet(np.ones(S), size=S)).astype(np.float32)
    init = np.log(rng.dirichlet(np.ones(S))).astype(np.float32)
    return obs, trans, init


def host(obs, frames, trans, init, weights=None):
    """The float64 route on log inputs: (gamma, L, X, I) as float64 tensors."""
    return training._host_counts(torch.as_tensor(obs), torch.as_tensor(frames), torch.as_tensor(trans),
                                 torch.as_tensor(init), None if weights is None else torch.as_tensor(weights))


@pytest.mark.parametrize('S', [2, 3, 4])
def test_float64_route_matches_brute_force(S):
    for T in range(1, 6):
        B = 4
        obs, trans, init = problem(B, T, S, seed=10 * S + T)
        frames = np.array([T, 1, max(1, T - 1), max(1, T - 2)], dtype=np.int32)
        weights = np.array([1., 0.5, 2., -0.25])
        _, L, X, I = host(obs, frames, trans, init, weights)
        rX, rI, rL = brute(obs, frames, trans, init, weights)
        assert np.abs(X.numpy() - rX).max() <= 1e-9
        assert np.abs(I.numpy() - rI).max() <= 1e-9
        assert np.abs(L.numpy() - rL).max() <= 1e-9
        # the public float32 entry: the same model through the epsilon round trip
        cX, cI, cL = torbi_amd.expected_counts(torch.as_tensor(obs), torch.as_tensor(frames), torch.as_tensor(trans),
                                               torch.as_tensor(init), log_probs=True)
        assert cX.dtype == cI.dtype == cL.dtype == torch.float32 and cX.shape == (S, S) and cI.shape == (S,)
        uX, uI, uL = brute(clamp(obs), frames, trans, init, np.ones(B))
        assert np.allclose(cX.numpy(), uX, rtol=1e-6, atol=1e-6) and np.allclose(cI.numpy(), uI, rtol=1e-6, atol=1e-6)
        assert np.allclose(cL.numpy(), uL, rtol=1e-6, atol=1e-5)


def test_single_frame_items_add_nothing_to_transition_counts():
    obs, trans, init = problem(3, 5, 3, seed=4)
    _, _, X, I = host(obs, np.ones(3, dtype=np.int32), trans, init)
    assert (X == 0).all() and abs(I.sum().item() - 3) <= 1e-12


def test_marginals_hold():
    B, T, S = 6, 9, 5
    obs, trans, init = problem(B, T, S, seed=7)
    frames = np.array([9, 1, 2, 5, 8, 3], dtype=np.int32)
    g = np.array([1., 2., 0.5, 0., 3., 1.5])
    gamma, _, X, I = host(obs, frames, trans, init, g)
    gamma, X = gamma.numpy(), X.numpy()
    t = np.arange(T)[None, :]
    before_last = (t < frames[:, None] - 1).astype(np.float64)          # t < F - 1
    after_first = ((t >= 1) & (t < frames[:, None])).astype(np.float64)  # 1 <= t < F
    assert np.allclose(X.sum(axis=0), np.einsum('b,bt,bti->i', g, before_last, gamma), atol=1e-12)
    assert np.allclose(X.sum(axis=1), np.einsum('b,bt,btj->j', g, after_first, gamma), atol=1e-12)
    assert abs(X.sum() - (g * (frames - 1)).sum()) <= 1e-11
    assert np.allclose(I.numpy(), np.einsum('b,bj->j', g, gamma[:, 0]), atol=1e-12)


def test_uniform_default_is_the_dense_route_on_a_filled_matrix():
    B, T, S = 3, 6, 4
    obs = torch.as_tensor(problem(B, T, S, seed=2)[0])
    X, I, L = torbi_amd.expected_counts(obs, log_probs=True)
    filled = torch.full((S, S), float(torch.tensor(math.log(1. / S), dtype=torch.float32)))
    X2, I2, L2 = torbi_amd.expected_counts(obs, None, filled, None, log_probs=True)
    assert torch.equal(X, X2) and torch.equal(I, I2) and torch.equal(L, L2)
    assert abs(X.sum().item() - B * (T - 1)) <= 1e-4


def test_likelihood_equals_state_posteriors_on_the_host_route():
    B, T, S = 5, 12, 6
    rng = np.random.default_rng(3)
    probs = torch.as_tensor(rng.dirichlet(np.ones(S), size=(B, T)).astype(np.float32))
    trans = torch.as_tensor(rng.dirichlet(np.ones(S), size=S).astype(np.float32))
    frames = torch.tensor([12, 1, 7, 3, 11], dtype=torch.int32)
    _, _, L = torbi_amd.expected_counts(probs, frames, trans)
    _, Lp = torbi_amd.state_posteriors(probs, frames, trans)
    assert torch.equal(L, Lp)


def _logsumexp_likelihood(obs, frames, trans, init):
    """Plain torch log-space forward recursion, differentiable by autograd."""
    B, T, S = obs.shape
    out = []
    for b in range(B):
        F = int(frames[b].clamp(1, T))
        la = init + obs[b, 0]
        for t in range(1, F):
            la = obs[b, t] + torch.logsumexp(trans + la[None, :], dim=1)
        out.append(torch.logsumexp(la, dim=0))
    return torch.stack(out)


def test_gradcheck_and_autograd_reference():
    B, T, S = 3, 4, 3
    obs, trans, init = (torch.as_tensor(x, dtype=torch.float64) for x in problem(B, T, S, seed=5))
    frames = torch.tensor([4, 1, 2], dtype=torch.int32)
    args = [obs.clone().requires_grad_(), frames, trans.clone().requires_grad_(), init.clone().requires_grad_()]
    assert torch.autograd.gradcheck(torbi_amd.log_likelihood, args, eps=1e-6, atol=1e-7)
    w = torch.tensor([0.7, -1.3, 2.1], dtype=torch.float64)
    L = torbi_amd.log_likelihood(*args)
    assert L.dtype == torch.float64
    (L * w).sum().backward()
    ref = [obs.clone().requires_grad_(), trans.clone().requires_grad_(), init.clone().requires_grad_()]
    Lr = _logsumexp_likelihood(ref[0], frames, ref[1], ref[2])
    assert torch.allclose(L, Lr, atol=1e-12)
    (Lr * w).sum().backward()
    for got, want in zip((args[0], args[2], args[3]), ref):
        assert torch.allclose(got.grad, want.grad, atol=1e-12), (got.grad - want.grad).abs().max()
    # rows t >= F_b get no gradient
    assert (args[0].grad[1, 1:] == 0).all() and (args[0].grad[2, 2:] == 0).all()


def test_float32_inputs_give_float32_results_and_gradients():
    obs, trans, init = (torch.as_tensor(x).requires_grad_() for x in problem(2, 5, 3, seed=9))
    L = torbi_amd.log_likelihood(obs, None, trans, init)
    assert L.dtype == torch.float32
    L.sum().backward()
    assert obs.grad.dtype == trans.grad.dtype == init.grad.dtype == torch.float32
    X, I, _ = torbi_amd.expected_counts(obs.detach(), None, trans.detach(), init.detach(), log_probs=True)
    # dL/dtransition is X, dL/dinitial is I; the counts entry clamps the observation, so compare loosely
    assert torch.allclose(trans.grad, X, atol=1e-5) and torch.allclose(init.grad, I, atol=1e-5)


def test_initial_gradient_alone_and_observation_gradient_alone():
    obs, trans, init = (torch.as_tensor(x, dtype=torch.float64) for x in problem(3, 6, 4, seed=11))
    frames = torch.tensor([6, 2, 4], dtype=torch.int32)
    full = [obs.clone().requires_grad_(), trans.clone().requires_grad_(), init.clone().requires_grad_()]
    torbi_amd.log_likelihood(full[0], frames, full[1], full[2]).sum().backward()
    i_only = init.clone().requires_grad_()
    torbi_amd.log_likelihood(obs, frames, trans, i_only).sum().backward()
    o_only = obs.clone().requires_grad_()
    torbi_amd.log_likelihood(o_only, frames, trans, init).sum().backward()
    assert torch.allclose(i_only.grad, full[2].grad, atol=1e-13) and torch.equal(o_only.grad, full[0].grad)


def test_nonfinite_items_are_skipped_and_the_autograd_nan_rule():
    B, T, S = 4, 6, 3
    obs, trans, init = (torch.as_tensor(x, dtype=torch.float64) for x in problem(B, T, S, seed=12))
    frames = torch.tensor([6, 5, 6, 3], dtype=torch.int32)
    bad = obs.clone()
    bad[1, 2, 0] = math.nan
    bad[3, 0, :] = -math.inf                                                   # total probability 0: L = -inf
    _, L, X, I = training._host_counts(bad, frames, trans, init, None)
    assert math.isnan(L[1]) and L[3] == -math.inf
    keep = torch.tensor([0, 2])
    _, L2, X2, I2 = training._host_counts(obs[keep], frames[keep], trans, init, None)
    assert torch.allclose(L[keep], L2, rtol=0, atol=1e-13) and torch.allclose(X, X2, atol=1e-13) and torch.allclose(I, I2, atol=1e-13)
    # a zero weight skips a NaN item (0 * NaN would poison the sum)
    _, _, X3, _ = training._host_counts(bad, frames, trans, init, torch.tensor([1., 0., 1., 0.]))
    assert torch.allclose(X3, X2, atol=1e-13)
    # autograd: a non-finite L with non-zero gradient makes the parameter gradients NaN ...
    t1, i1 = trans.clone().requires_grad_(), init.clone().requires_grad_()
    torbi_amd.log_likelihood(bad, frames, t1, i1).sum().backward()
    assert torch.isnan(t1.grad).all() and torch.isnan(i1.grad).all()
    # ... and with zero gradient on those items they are skipped
    t2, i2 = trans.clone().requires_grad_(), init.clone().requires_grad_()
    torbi_amd.log_likelihood(bad, frames, t2, i2)[keep].sum().backward()
    assert torch.allclose(t2.grad, X2, atol=1e-13) and torch.allclose(i2.grad, I2, atol=1e-13)


@pytest.mark.parametrize('gpu', [None, 0])
def test_misshaped_inputs_raise_before_any_work(gpu):
    B, T, S = 3, 4, 5
    obs = torch.from_numpy(synth.problem(B, T, S, seed=1)[0])
    trans, init = torch.zeros((S, S)), torch.zeros(S)
    frames = torch.full((B,), T, dtype=torch.int32)
    bad = [(dict(batch_frames=torch.tensor([5], dtype=torch.int32)), r'batch_frames must have shape \(3,\)'),
           (dict(initial=torch.zeros(1)), r'initial must have shape \(5,\)'),
           (dict(transition=torch.zeros((S - 1, S - 1))), r'transition must have shape \(5, 5\)')]
    for change, message in bad:
        args = dict(batch_frames=frames, transition=trans, initial=init)
        args.update(change)
        with pytest.raises(RuntimeError, match=message):
            torbi_amd.expected_counts(obs, log_probs=True, gpu=gpu, **args)
        with pytest.raises(RuntimeError, match=message):
            torbi_amd.forward_backward_counts(obs, args['batch_frames'], args['transition'], args['initial'])
        with pytest.raises(RuntimeError, match=message):
            torbi_amd.log_likelihood(obs if gpu is None else obs, args['batch_frames'], args['transition'], args['initial'])
    with pytest.raises(RuntimeError, match='item_weights must have shape'):
        torbi_amd.forward_backward_counts(obs, frames, trans, init, item_weights=torch.ones(B + 1))
    with pytest.raises(RuntimeError, match='observation must have shape'):
        torbi_amd.expected_counts(obs[0], gpu=gpu)


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    for name in ('torbi_hip_forward_backward_counts_workspace_bytes', 'torbi_hip_forward_backward_counts'):
        assert re.search(rf'\b{name}\s*\(', header) and name in _lib.SYMBOLS
    assert '#define TORBI_HIP_ABI_VERSION 17' in header and _lib.ABI_VERSION == 17
    for name in ('expected_counts', 'expected_counts_workspace_bytes', 'forward_backward_counts', 'log_likelihood'):
        assert name in torbi_amd.__all__ and callable(getattr(torbi_amd, name))


def test_c_abi_argument_errors_without_a_device():
    lib = _lib.load()
    B, T, S = 3, 5, 7
    need = lib.torbi_hip_forward_backward_counts_workspace_bytes(B, T, S)
    assert need == lib.torbi_hip_forward_backward_workspace_bytes(B, T, S)
    assert torbi_amd.expected_counts_workspace_bytes(B, T, S) == need
    p = ctypes.c_void_p(16)                  # never dereferenced: every call below fails its argument check first
    s = ctypes.c_void_p(0)
    fc = lib.torbi_hip_forward_backward_counts
    assert fc(p, p, p, p, p, p, p, p, p, p, need - 1, B, T, S, 0, s) == -2          # TORBI_HIP_EWORKSPACE
    assert fc(p, p, p, p, None, p, p, p, p, p, need - 1, B, T, S, 0, s) == -2       # (null weights are allowed)
    assert fc(p, p, p, p, p, p, p, p, p, p, need, B, 0, S, 0, s) == -1             # T < 1
    assert fc(p, p, p, p, p, p, p, p, p, p, need, B, T, 0, 0, s) == -1             # S < 1
    assert fc(p, p, p, p, p, p, p, p, p, p, need, -1, T, S, 0, s) == -1            # B < 0
    assert fc(p, p, p, p, p, p, p, p, p, None, need, B, T, S, 0, s) == -1          # null workspace
    assert fc(None, p, p, p, p, p, p, p, p, p, need, B, T, S, 0, s) == -1          # null observation
    assert fc(p, p, None, p, p, p, p, p, p, p, need, B, T, S, 0, s) == -1          # null transition
    assert fc(p, p, p, p, p, None, p, p, p, p, need, B, T, S, 0, s) == -1          # null posterior
    assert fc(p, p, p, p, p, p, None, p, p, p, need, B, T, S, 0, s) == -1          # null log-likelihood
    assert fc(p, p, p, p, p, p, p, None, p, p, need, B, T, S, 0, s) == -1          # null counts
    assert fc(p, p, p, p, p, p, p, p, None, p, need, B, T, S, 0, s) == -1          # null initial counts
    assert fc(p, p, p, p, p, p, p, p, p, p, 1 << 40, B, T, 20000, 0, s) == -3      # S beyond the build
    assert fc(None, None, None, None, None, None, None, None, None, None, 0, 0, T, S, 0, s) == 0   # B = 0


def sample_hmm(B, T, S, seed):
    """Sequences from a known HMM with Gaussian emissions; returns per-frame log emission likelihoods (B, T, S)."""
    rng = np.random.default_rng(seed)
    A = np.full((S, S), 0.1 / (S - 1)) + np.eye(S) * (0.9 - 0.1 / (S - 1))   # [next, prev], columns sum to 1
    pi = np.full(S, 1. / S)
    means = np.arange(S, dtype=np.float64) * 1.5
    states = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        s = rng.choice(S, p=pi)
        for t in range(T):
            if t:
                s = rng.choice(S, p=A[:, s])
            states[b, t] = s
    y = means[states] + rng.standard_normal((B, T))
    return (-0.5 * (y[..., None] - means) ** 2 - 0.5 * math.log(2 * math.pi)).astype(np.float32)


def em(obs, frames, steps, gpu):
    """Baum-Welch on transition and initial, emissions fixed: returns the total log-likelihood before each M-step."""
    S = obs.shape[2]
    rng = np.random.default_rng(0)
    trans = torch.log(torch.as_tensor(rng.dirichlet(np.ones(S), size=S).T.astype(np.float32)))   # columns sum to 1
    init = torch.full((S,), -math.log(S))
    totals = []
    for _ in range(steps):
        X, I, L = torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=gpu)
        totals.append(float(L.double().sum()))
        trans = torch.log(X / X.sum(dim=0, keepdim=True)).cpu()                 # M-step: normalise each column
        init = torch.log(I / I.sum()).cpu()
    return totals


def test_baum_welch_does_not_decrease_the_likelihood():
    obs = torch.as_tensor(sample_hmm(8, 40, 4, seed=1))
    frames = torch.tensor([40, 30, 40, 12, 40, 25, 40, 39], dtype=torch.int32)
    totals = em(obs, frames, 5, None)
    assert all(b >= a - 1e-6 * abs(a) for a, b in zip(totals, totals[1:])), totals
    assert totals[-1] > totals[0] + 1
