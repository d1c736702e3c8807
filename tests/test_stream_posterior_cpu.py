"""torbi_amd.StreamPosteriors without a device: the host route (`gpu=None`, float64) against `state_posteriors` on every
prefix and against path enumeration, its boundary and non-finite behaviour, and the surface of the C entry points
(torbi_hip_stream_posterior_*), whose argument checks run before any device work."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib
from stream_posterior_cases import HOST_GAMMA, Feeder, cpu, problem, ragged_plan, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('torbi_hip_stream_posterior_state_size', 'torbi_hip_stream_posterior_tile', 'torbi_hip_stream_posterior_push',
         'torbi_hip_stream_posterior_flush')
EINVAL, EWORKSPACE, ERANGE = -1, -2, -3
MAX_STATES = 8000


def feeder(B, S, kind, log_probs, lag, T, seed):
    obs, trans, init = problem(B, T, S, kind, log_probs, seed)
    sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=log_probs, gpu=None, lag=lag)
    return Feeder(sp, obs, trans, init, log_probs, HOST_GAMMA)


# ---- 1. the prefix property after every push ---------------------------------------------------------------------------

@pytest.mark.parametrize('lag', [0, 1, 3, 8])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('S', [1, 2, 3, 5, 17])
def test_prefix_property_after_every_push(S, B, lag):
    T = 24
    for k, (kind, log_probs) in enumerate(itertools.product(('none', 'dense', 'band'), (False, True))):
        fd = feeder(B, S, kind, log_probs, lag, T, seed=100 * S + 10 * B + lag + k)
        plan = ragged_plan(B, T, seed=S + B + lag + k)
        assert len(plan) >= 6 and any(Tc == 0 for Tc, _ in plan) and any(Tc == 7 for Tc, _ in plan)
        for Tc, f in plan:
            if B >= 2:
                assert (f == 0).any() and (f == Tc).any()
            fd.push(Tc, f)
        assert fd.sp.capacity <= lag + 7                     # the host route holds at most lag + Tc rows per stream
        fd.flush()


# ---- 2. brute force ----------------------------------------------------------------------------------------------------

def enumerate_posteriors(obs, trans, init):
    """gamma_{t|n} (n, S) and log P of a short sequence by enumerating all S^n paths in float64 (log inputs)."""
    n, S = obs.shape
    weight = np.zeros((n, S))
    total = 0.
    for path in itertools.product(range(S), repeat=n):
        logp = init[path[0]] + obs[0, path[0]]
        for t in range(1, n):
            logp += trans[path[t], path[t - 1]] + obs[t, path[t]]
        p = math.exp(logp)
        total += p
        for t in range(n):
            weight[t, path[t]] += p
    return weight / total, math.log(total)


@pytest.mark.parametrize('S,N,lag', [(2, 6, 0), (2, 6, 2), (3, 6, 1), (3, 5, 3), (3, 6, 5), (1, 4, 1)])
def test_one_frame_pushes_against_path_enumeration(S, N, lag):
    obs, trans, init = problem(1, N, S, 'dense', True, seed=S * N + lag)
    sp = torbi_amd.StreamPosteriors(1, S, trans, init, log_probs=True, gpu=None, lag=lag)
    fd = Feeder(sp, obs, trans, init, True, HOST_GAMMA)
    for _ in range(N):
        fd.push(1, check=False)
    fd.flush(check=False)
    assert sorted(t for _, t, _, _ in fd.returned) == list(range(N))
    o, A, pi = (x.numpy().astype(np.float64) for x in (obs[0], trans, init))
    for _, t, n, row in fd.returned:
        assert n == min(t + lag + 1, N)                   # exact fixed-lag smoothing, then the flush
        want, _ = enumerate_posteriors(o[:n], A, pi)
        same(row, want[t], HOST_GAMMA, f'gamma_{t}|{n}')
    # the running score against the enumeration, after every frame
    sp = torbi_amd.StreamPosteriors(1, S, trans, init, log_probs=True, gpu=None, lag=lag)
    for n in range(1, N + 1):
        sp.push(obs[:, n - 1:n])
        want, logp = enumerate_posteriors(o[:n], A, pi)
        assert abs(float(sp.log_likelihood[0]) - logp) <= 1e-6 * abs(logp) + 4e-6 * n
        same(cpu(sp.filtered())[0], want[n - 1], HOST_GAMMA, 'filtered')


# ---- 3. boundary behaviour ---------------------------------------------------------------------------------------------

def test_a_lag_beyond_the_sequence_returns_everything_at_the_flush():
    B, S, T = 2, 5, 11
    fd = feeder(B, S, 'dense', True, lag=T, T=T, seed=3)
    for Tc in (4, 1, 6):
        rows = fd.push(Tc)
        assert all(r.shape[0] == 0 for r in rows)
    rest, final = fd.flush()
    g, L = torbi_amd.state_posteriors(fd.obs, None, fd.trans, fd.init, log_probs=True, gpu=None)
    for b in range(B):
        same(cpu(rest[b]), g[b].numpy(), HOST_GAMMA, 'flush against the whole sequence')
    same(cpu(final), L.numpy(), 1e-6 * np.abs(L.numpy()) + 4e-6 * T, 'final log-likelihood')


def test_lag_zero_returns_every_frame_in_the_push_that_brought_it():
    fd = feeder(3, 4, 'band', False, lag=0, T=12, seed=4)
    for Tc, f in [(3, [3, 1, 0]), (1, [1, 1, 1]), (5, [0, 5, 2])]:
        rows = fd.push(Tc, f)
        assert [r.shape[0] for r in rows] == list(f)
    assert fd.sp.pending.tolist() == [0, 0, 0]
    rest, _ = fd.flush()
    assert all(r.shape[0] == 0 for r in rest)


def test_empty_pushes_and_a_second_flush():
    fd = feeder(2, 3, 'dense', True, lag=2, T=10, seed=5)
    rows = fd.push(0)                                         # Tc = 0 before anything else
    assert all(tuple(r.shape) == (0, 3) for r in rows)
    fd.push(4)
    before = (cpu(fd.sp.filtered()).copy(), cpu(fd.sp.log_likelihood).copy())
    fd.push(0)
    fd.push(3, [0, 0])
    assert np.array_equal(before[0], cpu(fd.sp.filtered())) and np.array_equal(before[1], cpu(fd.sp.log_likelihood))
    rest, final = fd.flush()
    assert [r.shape[0] for r in rest] == [2, 2]
    rest, final = fd.flush()                                  # nothing left: (0, S) rows and a log-likelihood of 0
    assert all(tuple(r.shape) == (0, 3) for r in rest) and final.tolist() == [0., 0.]
    assert (cpu(fd.sp.filtered()) == 0).all()


def test_flushing_no_stream_returns_nothing_before_and_after_a_push():
    """The host behaviour the device route matches (tests/test_stream_posterior_gpu.py): ([], tensor([])), nothing changes."""
    sp = torbi_amd.StreamPosteriors(2, 4, gpu=None, lag=1)
    for pushed in (0, 2):
        if pushed:
            sp.push(torch.rand((2, pushed, 4)))
        before = (sp.pending.tolist(), sp.frames.tolist(), sp.log_likelihood.clone())
        rest, final = sp.flush([])
        assert rest == [] and final.dtype == torch.float32 and tuple(final.shape) == (0,)
        assert (sp.pending.tolist(), sp.frames.tolist()) == before[:2] == ([min(pushed, 1)] * 2, [pushed] * 2)
        assert torch.equal(sp.log_likelihood, before[2])


def test_flushing_one_stream_half_way_restarts_it_from_initial():
    B, S, T = 3, 5, 14
    fd = feeder(B, S, 'dense', True, lag=3, T=T, seed=6)
    fd.push(4)
    fd.push(2, [2, 1, 2])
    rest, final = fd.flush(items=[1])
    assert rest[0].shape[0] == 3 and fd.sp.frames.tolist() == [6, 0, 6]
    fresh, _, _ = problem(1, 8, S, 'dense', True, seed=66)
    fd.restart(1, fresh[0])
    fd.push(5)                                                # stream 1 starts from `initial` again, its neighbours carry on
    fd.push(3, [3, 3, 0])
    fd.flush()
    with pytest.raises(IndexError):
        fd.sp.flush(items=[3])


# ---- 4. non-finite inputs ----------------------------------------------------------------------------------------------

def test_a_nan_observation_poisons_its_stream_until_the_flush():
    B, S, T, t0 = 3, 4, 16, 5
    obs, trans, init = problem(B, T, S, 'dense', True, seed=7)
    obs[1, t0, 2] = math.nan
    sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=True, gpu=None, lag=2)
    fd = Feeder(sp, obs, trans, init, True, HOST_GAMMA)
    fd.push(4)                                                # frames 0 .. 3: still clean
    assert not np.isnan(cpu(sp.log_likelihood)).any()
    for Tc in (3, 1, 4):                                      # frame t0 arrives; every later row of stream 1 is NaN
        rows = fd.push(Tc)
        assert np.isnan(cpu(rows[1])).all() and rows[1].shape[0] == Tc
        assert not np.isnan(cpu(rows[0])).any() and not np.isnan(cpu(rows[2])).any()
        assert np.isnan(cpu(sp.log_likelihood)).tolist() == [False, True, False]
        assert np.isnan(cpu(sp.filtered())[1]).all()
    rest, final = fd.flush(items=[1])
    assert np.isnan(cpu(rest[0])).all() and math.isnan(float(final[0]))
    clean, _, _ = problem(1, 4, S, 'dense', True, seed=77)
    fd.restart(1, clean[0])
    rows = fd.push(4)                                         # clean after the flush (checked against the reference)
    assert not np.isnan(cpu(rows[1])).any() and not np.isnan(cpu(sp.log_likelihood)).any()


def test_an_initial_without_mass_where_the_model_has_some_gives_minus_infinity():
    S, T = 4, 6
    obs, trans, _ = problem(2, T, S, 'band', True, seed=8)
    init = torch.full((S,), -math.inf)
    sp = torbi_amd.StreamPosteriors(2, S, trans, init, log_probs=True, gpu=None, lag=1)
    fd = Feeder(sp, obs, trans, init, True, HOST_GAMMA)
    for Tc in (2, 3, 1):
        rows = fd.push(Tc)
        assert all(np.isnan(cpu(r)).all() and r.shape[0] > 0 for r in rows)
        assert (cpu(sp.log_likelihood) == -math.inf).all()
    _, final = fd.flush()
    assert (cpu(final) == -math.inf).all()


# ---- 5. surface ------------------------------------------------------------------------------------------------------------

def test_the_class_is_exported_and_its_symbols_are_declared_within_abi_17():
    assert 'StreamPosteriors' in torbi_amd.__all__ and callable(torbi_amd.StreamPosteriors)
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(?:int|size_t) ' + name + r'\s*\(', header), name
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert not name.endswith('_bytes')
    declared = set(re.findall(r'\b(torbi_hip_stream_posterior_\w+)', header))
    assert declared == set(NAMES) == {n for n in _lib.SYMBOLS if n.startswith('torbi_hip_stream_posterior_')}
    assert '#define TORBI_HIP_ABI_VERSION 17' in header and _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17


def test_the_state_size_grows_with_every_argument_and_is_zero_for_a_non_positive_one():
    size = _lib.load().torbi_hip_stream_posterior_state_size
    B, S, cap = 3, 17, 16
    assert size(B, S, cap) == 8 * B + B * cap * (8 * S + 8)             # sums, a and e rows, c and m
    assert size(B + 1, S, cap) > size(B, S, cap) < size(B, S + 1, cap) and size(B, S, cap + 1) > size(B, S, cap)
    for bad in [(0, S, cap), (B, 0, cap), (B, S, 0), (-1, S, cap), (B, -5, cap), (B, S, -2)]:
        assert size(*bad) == 0
    assert size(512, 1440, 16) == 512 * (8 + 16 * (8 * 1440 + 8))
    assert size(4096, 8000, 64) == 4096 * (8 + 64 * (8 * 8000 + 8))    # beyond 2^32 bytes


def test_the_tile_query_answers_without_a_device_for_256_compute_units():
    tile = _lib.load().torbi_hip_stream_posterior_tile
    assert tile(0, 64, -1) == EINVAL and tile(4, 0, -1) == EINVAL and tile(1, MAX_STATES + 1, -1) == ERANGE
    # 16, halved while the workgroups are fewer than 256 compute units
    assert [tile(B, 64, -1) for B in (1, 510, 511, 1020, 1021, 2040, 2041, 4080, 4081)] == [1, 1, 2, 2, 4, 4, 8, 8, 16]
    assert tile(1 << 20, 512, -1) == 8 and tile(1 << 20, 2048, -1) == 2 and tile(1 << 20, MAX_STATES, -1) == 1


def test_the_entries_check_every_argument_before_any_device_work():
    lib = _lib.load()
    B, S, cap, out_cap, Tc = 2, 8, 16, 4, 3
    need = lib.torbi_hip_stream_posterior_state_size(B, S, cap)
    p = ctypes.c_void_p(4096)                                 # never dereferenced: every case below fails its checks

    def push(obs=p, Tc=Tc, info=p, expa=p, expa_t=p, initial=p, state=p, nbytes=need, cap=cap, out=p, out_cap=out_cap,
             counts=None, lag=2, B=B, S=S):
        return lib.torbi_hip_stream_posterior_push(obs, Tc, info, expa, expa_t, initial, state, nbytes, cap, out, out_cap, counts,
                                                   lag, B, S, 0, None)

    def flush(info=p, expa=p, state=p, nbytes=need, cap=cap, out=p, out_cap=out_cap, counts=None, B=B, S=S):
        return lib.torbi_hip_stream_posterior_flush(info, expa, state, nbytes, cap, out, out_cap, counts, B, S, 0, None)

    for bad in [dict(obs=None), dict(info=None), dict(expa=None), dict(expa_t=None), dict(initial=None), dict(state=None),
                dict(out=None), dict(B=0), dict(S=0), dict(B=-3), dict(cap=0), dict(out_cap=0), dict(lag=-1), dict(Tc=-1)]:
        assert push(**bad) == EINVAL, bad
    for bad in [dict(info=None), dict(expa=None), dict(state=None), dict(out=None), dict(B=0), dict(S=-1), dict(cap=0),
                dict(out_cap=0)]:
        assert flush(**bad) == EINVAL, bad
    big = lib.torbi_hip_stream_posterior_state_size(B, MAX_STATES + 1, cap)
    assert push(S=MAX_STATES + 1, nbytes=big) == ERANGE and flush(S=MAX_STATES + 1, nbytes=big) == ERANGE
    assert push(nbytes=need - 1) == EWORKSPACE and flush(nbytes=need - 1) == EWORKSPACE
    assert push(nbytes=0) == EWORKSPACE and push(cap=cap + 1) == EWORKSPACE


def test_the_constructor_turns_down_a_bad_lag_batch_or_states():
    for lag in (-1, 1.5, None, '3', True):
        with pytest.raises(ValueError):
            torbi_amd.StreamPosteriors(1, 3, gpu=None, lag=lag)
    for batch, states in [(0, 3), (1, 0), (-2, 4)]:
        with pytest.raises(ValueError):
            torbi_amd.StreamPosteriors(batch, states, gpu=None)
    with pytest.raises(ValueError):
        torbi_amd.StreamPosteriors(1, 3, torch.zeros(4, 4), gpu=None, log_probs=True)
    sp = torbi_amd.StreamPosteriors(2, 3, gpu=None)
    assert sp.lag == 8 and sp.frames.tolist() == [0, 0] and sp.pending.tolist() == [0, 0] and sp.capacity == 0
    with pytest.raises(ValueError):
        sp.push(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError):
        sp.push(torch.ones(2, 3, 3), torch.tensor([1, 4]))
    assert torbi_amd.StreamPosteriors.round_capacity(1) == 16 and torbi_amd.StreamPosteriors.round_capacity(48) == 64
