"""torbi_amd.state_posteriors on the host (gpu=None) against independent float64 log-space forward-backward and brute force,
and the C-ABI surface of the HIP route without a device."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = np.finfo(np.float32).tiny


def clamp(x):
    """from_probabilities' epsilon round trip on log inputs."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).clone()
    torch.exp_(t)
    t += torch.finfo(torch.float32).tiny
    torch.log_(t)
    return t.numpy()


def logsumexp(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.)
    with np.errstate(divide='ignore'):
        return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def reference(obs, frames, trans, init):
    """Log-space forward-backward with logaddexp (not scaled), float64: (gamma (B, T, S), L (B,))."""
    obs, trans, init = (np.asarray(x, dtype=np.float64) for x in (obs, trans, init))
    B, T, S = obs.shape
    gamma, L = np.zeros((B, T, S)), np.zeros(B)
    for b in range(B):
        F = int(min(max(frames[b], 1), T))
        la = np.zeros((F, S))
        la[0] = init + obs[b, 0]
        for t in range(1, F):
            la[t] = obs[b, t] + logsumexp(trans + la[t - 1][None, :], axis=1)
        lb = np.zeros((F, S))
        for t in range(F - 2, -1, -1):
            lb[t] = logsumexp(trans + (obs[b, t + 1] + lb[t + 1])[:, None], axis=0)
        L[b] = logsumexp(la[F - 1], axis=0)
        gamma[b, :F] = np.exp(la + lb - L[b])
    return gamma, L


def brute(obs, frames, trans, init):
    """Every path enumerated (tiny shapes)."""
    obs, trans, init = (np.asarray(x, dtype=np.float64) for x in (obs, trans, init))
    B, T, S = obs.shape
    gamma, L = np.zeros((B, T, S)), np.zeros(B)
    for b in range(B):
        F = int(min(max(frames[b], 1), T))
        total, marg = 0., np.zeros((F, S))
        for path in itertools.product(range(S), repeat=F):
            s = init[path[0]] + obs[b, 0, path[0]]
            for t in range(1, F):
                s += trans[path[t], path[t - 1]] + obs[b, t, path[t]]
            p = math.exp(s)
            total += p
            for t in range(F):
                marg[t, path[t]] += p
        L[b] = math.log(total)
        gamma[b, :F] = marg / total
    return gamma, L


def host(obs, frames, trans, init, log_probs=True):
    t = None if trans is None else torch.from_numpy(np.asarray(trans, dtype=np.float32))
    i = None if init is None else torch.from_numpy(np.asarray(init, dtype=np.float32))
    f = None if frames is None else torch.from_numpy(np.asarray(frames, dtype=np.int32))
    g, L = torbi_amd.state_posteriors(torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)), f, t, i,
                                      log_probs=log_probs, gpu=None)
    assert g.dtype == torch.float32 and L.dtype == torch.float32
    return g.numpy().astype(np.float64), L.numpy().astype(np.float64)


def close(got, want, frames, gtol=1e-6, ltol=1e-6):
    g, L = got
    rg, rL = want
    assert np.nanmax(np.abs(g - rg)) <= gtol
    F = np.clip(np.asarray(frames), 1, g.shape[1])
    assert np.all(np.abs(L - rL) <= ltol * np.abs(rL) + 4e-6 * F), (L, rL)


def test_against_log_space_reference():
    B, T, S = 5, 30, 24
    obs, trans, init = synth.problem(B, T, S, seed=3)
    trans = trans - logsumexp(trans.astype(np.float64), axis=0)[None, :].astype(np.float32)     # column-stochastic-ish
    frames = np.array([30, 1, 17, 29, 2], dtype=np.int32)
    got = host(obs, frames, trans, init)
    want = reference(clamp(obs), frames, trans, init)
    close(got, want, frames, gtol=1e-6)
    # gamma of the float64 route before the float32 cast is within ~1e-9; the cast itself is <= 6e-8
    assert np.abs(got[0] - want[0]).max() <= 1e-7
    assert (got[0][1, 1:] == 0).all() and (got[0][4, 2:] == 0).all()
    np.testing.assert_allclose(got[0][:, 0].sum(-1), 1, atol=1e-6)


@pytest.mark.parametrize('S,T', [(1, 1), (1, 5), (2, 6), (3, 4), (4, 3), (4, 1)])
def test_against_brute_force(S, T):
    obs, trans, init = synth.problem(3, T, S, seed=S * 10 + T)
    frames = np.array([T, max(1, T - 1), 1], dtype=np.int32)
    got = host(obs, frames, trans, init)
    want = brute(clamp(obs), frames, trans, init)
    close(got, want, frames)


def test_uniform_closed_form_matches_dense_route():
    B, T, S = 4, 12, 9
    obs, _, init = synth.problem(B, T, S, seed=5)
    frames = np.array([12, 5, 1, 11], dtype=np.int32)
    u = np.float32(math.log(1. / S))
    uniform = host(obs, frames, None, init)
    dense = host(obs, frames, np.full((S, S), u, dtype=np.float32), init)
    close(uniform, dense, frames)
    close(uniform, reference(clamp(obs), frames, np.full((S, S), u), init), frames)


def test_defaults_and_probabilities_match_from_probabilities_preprocessing():
    B, T, S = 2, 7, 5
    rng = np.random.default_rng(0)
    p = rng.random((B, T, S)).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    tp = rng.random((S, S)).astype(np.float32)
    tp /= tp.sum(0, keepdims=True)
    ip = np.full(S, 1. / S, dtype=np.float32)
    obs_t = torch.from_numpy(p.copy())
    g, L = torbi_amd.state_posteriors(obs_t, None, torch.from_numpy(tp), torch.from_numpy(ip), gpu=None)
    assert torch.equal(obs_t, torch.from_numpy(p))                           # the caller's tensor is not written
    lo = clamp(torch.log(torch.from_numpy(p)).numpy())
    want = reference(lo, [T] * B, torch.log(torch.from_numpy(tp)).numpy(), torch.log(torch.from_numpy(ip)).numpy())
    close((g.numpy().astype(np.float64), L.numpy().astype(np.float64)), want, [T] * B)
    # no initial, no transition: log(1/S + tiny) and the uniform log(1/S)
    g2, L2 = torbi_amd.state_posteriors(torch.from_numpy(p), gpu=None)
    init = np.full(S, np.float32(math.log(1. / S + TINY)))
    want2 = reference(lo, [T] * B, np.full((S, S), np.float32(math.log(1. / S))), init)
    close((g2.numpy().astype(np.float64), L2.numpy().astype(np.float64)), want2, [T] * B)


def _model_entry(entry, obs, trans, init, log_probs):
    """One call of an entry point that prepares its inputs like from_probabilities (gpu=None); its outputs as a list."""
    B, _, S = obs.shape
    if entry == 'from_probabilities':
        return [torbi_amd.from_probabilities(obs, None, trans, init, log_probs=log_probs)]
    if entry == 'StreamDecoder':
        dec = torbi_amd.StreamDecoder(B, S, trans, init, log_probs=log_probs, gpu=None)
        return dec.push(obs) + dec.flush()
    return list(getattr(torbi_amd, entry)(obs, None, trans, init, log_probs=log_probs))


@pytest.mark.parametrize('entry,log_probs,written', [('from_probabilities', True, True),
                                                     ('from_probabilities', False, False),
                                                     ('StreamDecoder', True, False), ('state_posteriors', True, False),
                                                     ('expected_counts', True, False)])
def test_only_from_probabilities_writes_the_callers_observation(entry, log_probs, written):
    """from_probabilities takes a float32 log observation on the compute device through the epsilon round trip in place,
    like upstream; the other entry points work on a copy."""
    obs, trans, init = (torch.from_numpy(x) for x in synth.problem(2, 6, 5, seed=21))
    obs[0, 0, 0] = -math.inf                          # log(exp(x) + tiny) != x here
    if not log_probs:
        obs, trans, init = obs.exp(), trans.exp(), init.exp()
    kept = obs.clone()
    _model_entry(entry, obs, trans, init, log_probs)
    assert torch.equal(obs, kept) != written


@pytest.mark.parametrize('entry', ['from_probabilities', 'StreamDecoder', 'state_posteriors', 'expected_counts'])
def test_a_float64_initial_is_cast_except_by_from_probabilities(entry):
    """from_probabilities hands a float64 initial to the operator, which rejects it (like upstream); the other entry
    points cast it to float32."""
    obs, trans, init = (torch.from_numpy(x) for x in synth.problem(3, 8, 6, seed=22))
    if entry == 'from_probabilities':
        with pytest.raises(RuntimeError, match='initial'):
            _model_entry(entry, obs, trans, init.double(), True)
        return
    got = _model_entry(entry, obs, trans, init.double(), True)
    want = _model_entry(entry, obs, trans, init, True)
    assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))


def test_ragged_and_out_of_range_frames():
    B, T, S = 4, 9, 6
    obs, trans, init = synth.problem(B, T, S, seed=9)
    frames = np.array([0, -3, 100, 4], dtype=np.int32)
    got = host(obs, frames, trans, init)
    want = reference(clamp(obs), frames, trans, init)
    close(got, want, frames)
    assert (got[0][0, 1:] == 0).all() and (got[0][1, 1:] == 0).all() and (got[0][3, 4:] == 0).all()


@pytest.mark.parametrize('tiny', [False, True])
def test_banded_pitch_matrices(tiny):
    B, T, S = 3, 25, 40
    obs, _, init = synth.problem(B, T, S, seed=11)
    trans = synth.banded_transition(S, 4, tiny=tiny)
    init = np.log(np.full(S, 1. / S, dtype=np.float32))
    frames = np.array([25, 13, 1], dtype=np.int32)
    got = host(obs, frames, trans, init)
    want = reference(clamp(obs), frames, trans, init)
    close(got, want, frames)


def test_nonfinite_rules():
    B, T, S = 5, 6, 4
    obs, trans, init = synth.problem(B, T, S, seed=2)
    obs = obs.copy()
    frames = np.array([6, 6, 6, 6, 3], dtype=np.int32)
    obs[1, 3, 2] = np.nan             # NaN read
    obs[2, 4, 0] = np.inf             # +inf read
    obs[3, 2, :] = -np.inf            # log(0 + tiny) after the epsilon round trip: small, not zero
    obs[4, 5, 1] = np.nan             # beyond the item's frames: not read
    g, L = host(obs, frames, trans, init)
    clean = host(np.where(np.arange(B)[:, None, None] == 0, obs, obs[0:1]), frames, trans, init)
    assert np.isnan(L[1]) and np.isnan(g[1]).all()
    assert np.isnan(L[2]) and np.isnan(g[2]).all()
    assert np.isfinite(L[3]) and np.isfinite(g[3]).all()
    assert np.isfinite(L[4]) and np.isfinite(g[4, :3]).all() and (g[4, 3:] == 0).all()
    assert np.array_equal(g[0], clean[0][0]) and L[0] == clean[1][0]      # other items are not affected
    # total probability 0 (no transition allowed): L = -inf and NaN rows; one frame needs no transition
    never = np.full((S, S), -np.inf, dtype=np.float32)
    g2, L2 = host(obs[0:2], [6, 1], never, init)
    assert L2[0] == -np.inf and np.isnan(g2[0]).all()
    close((g2[1:], L2[1:]), reference(clamp(obs[1:2]), [1], never, init), [1])
    # ... and a NaN read after the zero-probability frame still gives NaN
    o2 = obs[0:1].copy()
    o2[0, 4, 1] = np.nan
    g2, L2 = host(o2, [6], never, init)
    assert np.isnan(L2[0]) and np.isnan(g2).all()
    g2, L2 = host(obs[0:1], [6], trans, np.full(S, -np.inf, dtype=np.float32))
    assert L2[0] == -np.inf and np.isnan(g2).all()
    # -inf initial entries and masked observations are ordinary zeros
    init2 = init.copy()
    init2[0] = -np.inf
    o3 = obs[0:1].copy()
    o3[0, :, 3] = -np.inf
    close(host(o3, [6], trans, init2), reference(clamp(o3), [6], trans, init2), [6])
    # a NaN or +inf in the transition matrix affects every item that takes a step
    for bad in (np.nan, np.inf):
        t2 = trans.copy()
        t2[1, 2] = bad
        g3, L3 = host(obs[0:2], [6, 6], t2, init)
        assert np.isnan(L3).all() and np.isnan(g3).all()


def test_single_frame_and_single_state():
    obs, trans, init = synth.problem(2, 1, 7, seed=4)
    close(host(obs, None, trans, init), brute(clamp(obs), [1, 1], trans, init), [1, 1])
    obs, trans, init = synth.problem(2, 8, 1, seed=4)
    g, L = host(obs, None, trans, init)
    assert (g == 1).all()
    want = init[0] + clamp(obs)[:, :, 0].astype(np.float64).sum(1) + 7 * np.float64(trans[0, 0])
    np.testing.assert_allclose(L, want, rtol=1e-6)


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    for name in ('torbi_hip_forward_backward_workspace_bytes', 'torbi_hip_forward_backward',
                 'torbi_hip_forward_backward_uniform'):
        assert re.search(rf'\b{name}\s*\(', header) and name in _lib.SYMBOLS
    assert '#define TORBI_HIP_ABI_VERSION 17' in header and _lib.ABI_VERSION == 17
    lib = _lib.load()
    assert lib.torbi_hip_abi_version() == 17
    for name in ('state_posteriors', 'forward_backward', 'forward_backward_workspace_bytes'):
        assert name in torbi_amd.__all__ and callable(getattr(torbi_amd, name))


def test_c_abi_argument_errors_without_a_device():
    lib = _lib.load()
    B, T, S = 3, 5, 7
    need = lib.torbi_hip_forward_backward_workspace_bytes(B, T, S)
    assert need >= 2 * 8 * 64 * 4 and torbi_amd.forward_backward_workspace_bytes(B, T, S) == need
    assert lib.torbi_hip_forward_backward_workspace_bytes(B, T, 100) > need
    p = ctypes.c_void_p(16)                  # never dereferenced: every call below fails its argument check first
    s = ctypes.c_void_p(0)
    fb, fbu = lib.torbi_hip_forward_backward, lib.torbi_hip_forward_backward_uniform
    for call in (lambda *a: fb(*a), lambda *a: fbu(a[0], a[1], ctypes.c_float(-1.), *a[3:])):
        assert call(p, p, p, p, p, p, p, need - 1, B, T, S, 0, s) == -2           # TORBI_HIP_EWORKSPACE
        assert call(p, p, p, p, p, p, p, need, B, 0, S, 0, s) == -1               # T < 1
        assert call(p, p, p, p, p, p, p, need, B, T, 0, 0, s) == -1               # S < 1
        assert call(p, p, p, p, p, p, p, need, -1, T, S, 0, s) == -1              # B < 0
        assert call(p, p, p, p, p, p, None, need, B, T, S, 0, s) == -1            # null workspace
        assert call(None, p, p, p, p, p, p, need, B, T, S, 0, s) == -1            # null observation
        assert call(p, p, p, p, None, p, p, need, B, T, S, 0, s) == -1            # null posterior
        assert call(p, p, p, p, p, None, p, need, B, T, S, 0, s) == -1            # null log-likelihood
        assert call(p, p, p, p, p, p, p, 1 << 40, B, T, 20000, 0, s) == -3        # S beyond the build
        assert call(None, None, None, None, None, None, None, 0, 0, T, S, 0, s) == 0   # B = 0: nothing to do
    assert fb(p, p, None, p, p, p, p, need, B, T, S, 0, s) == -1                  # null transition


@pytest.mark.parametrize('gpu', [None, 0])
def test_misshaped_inputs_raise_before_any_work(gpu):
    """batch_frames (B,), transition (S, S) and initial (S,) are checked on both routes (the GPU route raises before it
    asks for a device), and at the operator level."""
    B, T, S = 3, 4, 5
    obs = torch.from_numpy(synth.problem(B, T, S, seed=1)[0])
    trans, init = torch.zeros((S, S)), torch.zeros(S)
    frames = torch.full((B,), T, dtype=torch.int32)
    bad = [(dict(batch_frames=torch.tensor([5], dtype=torch.int32)), r'batch_frames must have shape \(3,\)'),
           (dict(batch_frames=torch.full((B, 1), T, dtype=torch.int32)), 'batch_frames must have shape'),
           (dict(initial=torch.zeros(1)), r'initial must have shape \(5,\)'),
           (dict(transition=torch.zeros((S - 1, S - 1))), r'transition must have shape \(5, 5\)'),
           (dict(transition=torch.zeros((S, S - 1))), 'transition must have shape')]
    for change, message in bad:
        args = dict(batch_frames=frames, transition=trans, initial=init)
        args.update(change)
        with pytest.raises(RuntimeError, match=message):
            torbi_amd.state_posteriors(obs, log_probs=True, gpu=gpu, **args)
        with pytest.raises(RuntimeError, match=message):
            torbi_amd.forward_backward(obs, args['batch_frames'], args['transition'], args['initial'])
    with pytest.raises(RuntimeError, match='initial must have shape'):
        torbi_amd.state_posteriors(obs, None, None, torch.zeros(S + 1), log_probs=True, gpu=gpu)   # uniform route
    with pytest.raises(RuntimeError, match='observation must have shape'):
        torbi_amd.state_posteriors(obs[0], gpu=gpu)
