"""k-best Viterbi decoding on the host route (torbi_amd/k_best.py) against brute-force enumeration and the existing decoders,
its edge rules, and the C-ABI surface of the HIP route without a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import _lib, synth
from k_best_cases import brute, same, clamp, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(obs, frames, trans, init, k):
    t = None if trans is None else torch.as_tensor(trans)
    i, s = torbi_amd.best_paths(torch.as_tensor(obs), k, None if frames is None else torch.as_tensor(frames), t,
                                torch.as_tensor(init), log_probs=True, gpu=None)
    assert i.dtype == torch.int32 and s.dtype == torch.float32 and i.shape == (obs.shape[0], k, obs.shape[1])
    return i.numpy(), s.numpy()


@pytest.mark.parametrize('S,T,B,seed', [(S, T, B, seed) for (S, T, B, seed) in
                                        [(1, 6, 2, 0), (2, 6, 3, 1), (3, 5, 3, 2), (4, 4, 3, 3), (2, 1, 2, 4), (3, 6, 2, 5),
                                         (4, 5, 2, 6)]])
@pytest.mark.parametrize('k', [1, 2, 3, 7, 16])
@pytest.mark.parametrize('ties', [False, True])
def test_against_brute_force(S, T, B, seed, k, ties):
    obs, trans, init = model(B, T, S, seed, ties)
    frames = np.array([T] + [max(1, T - 2 - b) for b in range(B - 1)], dtype=np.int32)
    same(host(obs, frames, trans, init, k), brute(clamp(obs), frames, trans, init, k))


@pytest.mark.parametrize('ties', [False, True])
def test_neg_inf_entries_against_brute_force(ties):
    B, T, S, k = 3, 5, 4, 16
    obs, trans, init = model(B, T, S, 7, ties)
    trans[0, :] = -np.inf           # nothing enters state 0 after frame 0
    trans[2, 1] = -np.inf
    init[3] = -np.inf
    frames = np.array([5, 3, 1], dtype=np.int32)
    got = host(obs, frames, trans, init, k)
    same(got, brute(clamp(obs), frames, trans, init, k))
    assert np.isneginf(got[1][2, 3]) and (got[0][2, 3] == 3).all()        # a real -inf path keeps its indices
    assert np.isneginf(got[1][2, 4:]).all() and (got[0][2, 4:] == -1).all()   # missing ranks


def test_more_ranks_than_paths():
    B, T, S, k = 2, 2, 3, 16                     # 9 paths
    obs, trans, init = model(B, T, S, 8, False)
    frames = np.array([2, 1], dtype=np.int32)    # 9 and 3 paths
    i, s = host(obs, frames, trans, init, k)
    same((i, s), brute(clamp(obs), frames, trans, init, k))
    assert np.isneginf(s[0, 9:]).all() and (i[0, 9:] == -1).all() and np.isfinite(s[0, :9]).all()
    assert np.isneginf(s[1, 3:]).all() and (i[1, 3:] == -1).all()
    assert (i[1, :3, 1] == i[1, :3, 0]).all()    # padding repeats the last state


def test_paths_are_distinct_and_scores_do_not_increase():
    B, T, S, k = 4, 12, 5, 32
    obs, trans, init = model(B, T, S, 9, True)
    i, s = host(obs, None, trans, init, k)
    assert (s[:, :-1] >= s[:, 1:]).all()
    for b in range(B):
        assert len({tuple(p) for p in i[b]}) == k


def _golden_cases(golden):
    for name in golden.small_names():
        obs, frames, trans, init, want = golden.small_case(name)
        if obs.ndim != 3 or not all(np.all(x < np.inf) for x in (obs, trans, init)):
            continue
        yield name, obs.astype(np.float32), frames.astype(np.int32), trans.astype(np.float32), init.astype(np.float32)


def _rank_zero(obs, frames, trans, init, k):
    i, s = torbi_amd.decode_k_best(torch.as_tensor(obs), torch.as_tensor(frames), torch.as_tensor(trans),
                                   torch.as_tensor(init), k)
    want, post = oracle.decode(obs, frames, trans, init, num_threads=2, return_posterior=True)
    assert np.array_equal(i[:, 0].numpy(), want)
    twin = torbi_amd.decode_cpu(torch.as_tensor(obs), torch.as_tensor(frames), torch.as_tensor(trans),
                                torch.as_tensor(init))
    assert np.array_equal(i[:, 0].numpy(), twin.numpy())
    assert np.array_equal(s[:, 0].numpy().view(np.int32), post.max(axis=1).view(np.int32))


def test_rank_zero_is_the_decoder_on_golden_cases(golden):
    seen = 0
    for name, obs, frames, trans, init in _golden_cases(golden):
        _rank_zero(obs, frames, trans, init, 3)
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize('B,T,S,k', [(4, 30, 40, 4), (3, 20, 97, 2), (2, 12, 360, 1), (5, 9, 7, 32)])
def test_rank_zero_is_the_decoder_on_synthetic_problems(B, T, S, k):
    obs, trans, init = synth.problem(B, T, S, seed=B * T + S)
    frames = np.clip(synth.lengths(B, 1, T, seed=S), 1, T).astype(np.int32)
    frames[0] = T
    _rank_zero(obs, frames, trans, init, k)


def test_rank_zero_is_from_probabilities():
    B, T, S = 3, 15, 9
    rng = np.random.default_rng(4)
    p = torch.tensor(rng.random((B, T, S), dtype=np.float32))
    A = torch.tensor(rng.random((S, S), dtype=np.float32))
    pi = torch.tensor(rng.random(S, dtype=np.float32))
    frames = torch.tensor([15, 6, 1])
    for trans, initial in ((A, pi), (None, None)):
        want = torbi_amd.from_probabilities(p, frames, trans, initial, gpu=None)
        i, _ = torbi_amd.best_paths(p, 4, frames, trans, initial, gpu=None)
        assert torch.equal(i[:, 0].to(want.dtype), want)


def test_uniform_route_equals_the_fill_matrix():
    B, T, S, k = 3, 6, 4, 7
    obs, _, init = model(B, T, S, 10, True)
    fill = torch.full((S, S), math.log(1. / S), dtype=torch.float32).numpy()
    same(host(obs, None, None, init, k), host(obs, None, fill, init, k))
    same(host(obs, None, None, init, k), brute(clamp(obs), [T] * B, fill, init, k))


def test_nonfinite_items_are_flagged_and_isolated():
    B, T, S, k = 5, 6, 3, 4
    obs, trans, init = model(B, T, S, 11, False)
    frames = np.array([6, 6, 3, 6, 6], dtype=np.int32)
    obs[1, 2, 1] = np.nan
    obs[2, 4, 0] = np.inf          # beyond its frames: not read
    obs[3, 0, 2] = np.inf
    i, s = torbi_amd.decode_k_best(torch.tensor(obs), torch.tensor(frames), torch.tensor(trans), torch.tensor(init), k)
    i, s = i.numpy(), s.numpy()
    assert np.isnan(s[[1, 3]]).all() and (i[[1, 3]] == -1).all()
    clean = [0, 2, 4]
    want = brute(obs[clean], frames[clean], trans, init, k)
    same((i[clean], s[clean]), want)
    # the matrix is read only by items with two frames or more; initial by every item
    bad = trans.copy()
    bad[1, 2] = np.nan
    frames = np.array([6, 1, 1, 2, 6], dtype=np.int32)
    i, s = torbi_amd.decode_k_best(torch.zeros(obs.shape), torch.tensor(frames), torch.tensor(bad), torch.tensor(init), k)
    assert np.isnan(s.numpy()[[0, 3, 4]]).all() and np.isfinite(s.numpy()[[1, 2], :3]).all()
    badi = init.copy()
    badi[0] = np.inf
    _, s = torbi_amd.decode_k_best(torch.zeros(obs.shape), torch.tensor(frames), torch.tensor(trans), torch.tensor(badi), k)
    assert np.isnan(s.numpy()).all()


@pytest.mark.parametrize('k', [0, 33, -1, 2.0, True])
def test_k_outside_the_range_raises(k):
    obs, trans, init = model(1, 3, 2, 0, False)
    with pytest.raises(RuntimeError, match='k must be'):
        torbi_amd.best_paths(torch.tensor(obs), k, transition=torch.tensor(trans), log_probs=True)
    with pytest.raises(RuntimeError, match='k must be'):
        torbi_amd.decode_k_best(torch.tensor(obs), None, torch.tensor(trans), torch.tensor(init), k)


@pytest.mark.parametrize('gpu', [None, 0])
def test_misshaped_inputs_raise_before_any_work(gpu):
    obs = torch.zeros((2, 4, 3))
    with pytest.raises(RuntimeError, match='batch_frames must have shape'):
        torbi_amd.best_paths(obs, 2, torch.tensor([4, 4, 4]), gpu=gpu)
    with pytest.raises(RuntimeError, match='transition must have shape'):
        torbi_amd.best_paths(obs, 2, transition=torch.ones((3, 4)), gpu=gpu)
    with pytest.raises(RuntimeError, match='initial must have shape'):
        torbi_amd.best_paths(obs, 2, initial=torch.ones(4), gpu=gpu)
    with pytest.raises(RuntimeError, match='observation must have shape'):
        torbi_amd.best_paths(obs[0], 2, gpu=gpu)


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    for name in ('torbi_hip_k_best_workspace_bytes', 'torbi_hip_k_best', 'torbi_hip_k_best_uniform'):
        assert re.search(rf'\b{name}\s*\(', header) and name in _lib.SYMBOLS
    assert '#define TORBI_HIP_ABI_VERSION 17' in header and _lib.ABI_VERSION == 17
    lib = _lib.load()
    assert lib.torbi_hip_abi_version() == 17
    for name in ('best_paths', 'decode_k_best', 'decode_k_best_workspace_bytes'):
        assert name in torbi_amd.__all__ and callable(getattr(torbi_amd, name))


def test_c_abi_argument_errors_without_a_device():
    lib = _lib.load()
    B, T, S, k = 3, 5, 7, 4
    need = lib.torbi_hip_k_best_workspace_bytes(B, T, S, k)
    assert need >= 4 * B * (T - 1) * k * S and torbi_amd.decode_k_best_workspace_bytes(B, T, S, k) == need
    assert lib.torbi_hip_k_best_workspace_bytes(B, T, 1, k) < need
    p = ctypes.c_void_p(16)                  # never dereferenced: every call below fails its argument check first
    st = ctypes.c_void_p(0)
    kb, kbu = lib.torbi_hip_k_best, lib.torbi_hip_k_best_uniform
    for call, n in ((lambda *a: kb(*a), need),
                    (lambda *a: kbu(a[0], a[1], ctypes.c_float(-1.), *a[3:]), lib.torbi_hip_k_best_workspace_bytes(B, T, 1, k))):
        assert call(p, p, p, p, p, p, p, n - 1, B, T, S, k, 0, st) == -2          # TORBI_HIP_EWORKSPACE
        assert call(p, p, p, p, p, p, p, n, B, 0, S, k, 0, st) == -1              # T < 1
        assert call(p, p, p, p, p, p, p, n, B, T, 0, k, 0, st) == -1              # S < 1
        assert call(p, p, p, p, p, p, p, n, -1, T, S, k, 0, st) == -1             # B < 0
        assert call(p, p, p, p, p, p, p, n, B, T, S, 0, 0, st) == -1              # k < 1
        assert call(p, p, p, p, p, p, p, n, B, T, S, 33, 0, st) == -1             # k > 32
        assert call(p, p, p, p, p, p, None, n, B, T, S, k, 0, st) == -1           # null workspace
        assert call(None, p, p, p, p, p, p, n, B, T, S, k, 0, st) == -1           # null observation
        assert call(p, p, p, p, None, p, p, n, B, T, S, k, 0, st) == -1           # null indices
        assert call(p, p, p, p, p, None, p, n, B, T, S, k, 0, st) == -1           # null scores
        assert call(p, p, p, p, p, p, p, 1 << 40, B, T, 20000, k, 0, st) == -3    # S beyond the build
        assert call(None, None, None, None, None, None, None, 0, 0, T, S, k, 0, st) == 0   # B = 0: nothing to do
    assert kb(p, p, None, p, p, p, p, need, B, T, S, k, 0, st) == -1             # null transition


def test_host_route_chunks_over_items_and_states(monkeypatch):
    """A chunk bound smaller than one item's candidates of one next-state still gives the same bits: the host route
    splits over items and over next-states."""
    from torbi_amd import k_best
    B, T, S, k = 7, 6, 5, 4
    obs, trans, init = model(B, T, S, 12, True)
    frames = np.array([6, 1, 3, 6, 2, 5, 4], dtype=np.int32)
    want = host(obs, frames, trans, init, k)
    for chunk in (1, 7, 64):
        monkeypatch.setattr(k_best, '_HOST_CHUNK_ELEMENTS', chunk)
        same(host(obs, frames, trans, init, k), want)
    same(want, brute(clamp(obs), frames, trans, init, k))


def test_uniform_workspace_size():
    B, T, S, k = 4, 9, 300, 5
    lib = _lib.load()
    assert torbi_amd.decode_k_best_workspace_bytes(B, T, S, k) == lib.torbi_hip_k_best_workspace_bytes(B, T, S, k)
    small = torbi_amd.decode_k_best_workspace_bytes(B, T, S, k, uniform=True)
    assert small == lib.torbi_hip_k_best_workspace_bytes(B, T, 1, k)
    assert small < torbi_amd.decode_k_best_workspace_bytes(B, T, S, k)
    assert small >= 4 * B * (T - 1) * k
