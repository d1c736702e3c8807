"""Path entropy without a device (torbi_amd/entropy.py, ENTROPY.md): the float64 host route against the three float64
references of tests/path_entropy_cases.py -- enumeration of every path, the recursion as a numpy loop, and the identity
H = L - E[log weight] through forward-backward --, every prefix entry, the bound by the frame entropies, the cases whose
entropy is 0, the uniform collapse, the non-finite rules, `log_probs` both ways, the C-ABI surface, the argument checks and
the workspace's layout.  tests/test_path_entropy_gpu.py runs the device routes against the same host route."""
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, entropy, inputs

import operand_form_cases as ofc
import path_entropy_cases as pec

CPU = torch.device('cpu')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('torbi_hip_path_entropy_workspace_size', 'torbi_hip_path_entropy', 'torbi_hip_path_entropy_uniform')


def host64(obs, frames, A, pi):
    """(H, L, prefix) of the host route before it is rounded to float32."""
    o, f, a, p = pec.tensors(obs, frames, A, pi)
    uniform = None if A is not None else float(pec.uniform_value(np.asarray(obs).shape[2]))
    return tuple(x.numpy() for x in entropy._host(o, f, a, uniform, p))


def words(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32 if x.dtype == np.float32 else np.int64)


# ------------------------------------------------------------------------------------------------ against the references
@pytest.mark.parametrize('matrix', pec.KINDS, ids=[str(k) for k in pec.KINDS])
@pytest.mark.parametrize('S,T', pec.ENUMERATED, ids=[f'S{S}-T{T}' for S, T in pec.ENUMERATED])
def test_host_route_equals_the_three_references(S, T, matrix):
    obs, frames, A, pi, want = pec.enumerated_case(S, T, matrix)
    assert frames[0] == T and frames[-1] == 1                   # ragged, F = 1 included
    H, L, prefix = host64(obs, frames, A, pi)
    for name, ref in (('enumeration', want), ('loop', pec.loop(obs, frames, A, pi)), ('identity', pec.identity(obs, frames, A, pi))):
        pec.close(H, ref[0], pec.reference_bound(ref[0]), (name, 'H'))
        pec.close(L, ref[1], pec.reference_bound(ref[1]), (name, 'L'))
        if len(ref) > 2:
            pec.close(prefix, ref[2], pec.reference_bound(ref[2]), (name, 'every prefix entry'))
    F = pec.clamp(frames, T)
    assert all((prefix[b, F[b]:] == 0).all() and prefix[b, F[b] - 1] == H[b] for b in range(len(F)))
    if matrix in ('left_to_right', 'permutation') and S > 1:
        assert np.isneginf(A).any()
    assert np.isfinite(H).all() and np.isfinite(prefix).all()  # a state no path reaches makes no NaN


@pytest.mark.parametrize('B,T,S,matrix', [(3, 50, 200, 'dense'), (4, 30, 65, 'left_to_right'), (3, 12, 33, 'permutation'),
                                          (3, 20, 70, None)])
def test_host_route_equals_loop_and_identity_on_larger_shapes(B, T, S, matrix):
    obs, frames, A, pi = pec.softmax_case(B, T, S, 7 * S + T, matrix=matrix)
    H, L, prefix = host64(obs, frames, A, pi)
    want = pec.loop(obs, frames, A, pi)
    for got, ref, name in zip((H, L, prefix), want, ('H', 'L', 'prefix')):
        pec.close(got, ref, pec.reference_bound(ref), ('loop', name))
    other = pec.identity(obs, frames, A, pi)
    pec.close(H, other[0], pec.reference_bound(other[0]), 'identity')
    # H <= the sum of the frame entropies of the posteriors
    assert (H <= pec.frame_entropies(obs, frames, A, pi) + pec.reference_bound(H)).all()
    assert (np.diff(np.concatenate([np.zeros((B, 1)), prefix], 1), axis=1)[:, 0] >= 0).all() and (H >= -pec.reference_bound(H)).all()


def test_the_public_routes_round_the_float64_values_once():
    obs, frames, A, pi = pec.softmax_case(3, 9, 33, 5)
    H, L, prefix = host64(obs, frames, A, pi)
    got = entropy.forward_entropy(*pec.tensors(obs, frames, A, pi), prefix=True)
    assert all(x.dtype == torch.float32 and x.device == CPU for x in got)
    for g, w in zip(got, (H, L, prefix)):
        assert np.array_equal(g.numpy(), w.astype(np.float32))
    short = entropy.forward_entropy(*pec.tensors(obs, frames, A, pi))
    assert len(short) == 2 and torch.equal(short[0], got[0]) and torch.equal(short[1], got[1])


# ------------------------------------------------------------------------------------------------ entropy 0
def test_one_state_has_entropy_zero():
    for matrix in ('dense', None):
        obs, frames, A, pi = pec.softmax_case(3, 4, 1, 2, matrix=matrix)
        H, L, prefix = host64(obs, frames, A, pi)
        assert (H == 0).all() and (prefix == 0).all() and np.isfinite(L).all()


def test_a_permutation_matrix_keeps_the_entropy_of_the_first_frame():
    B, T, S = 3, 12, 33
    obs, frames, A, pi = pec.softmax_case(B, T, S, 7 * S + T, matrix='permutation')
    H, L, prefix = host64(obs, frames, A, pi)
    # the path is a function of q_0, so prefix_t is the entropy of q_0 given o_0 .. o_t; with a constant observation behind
    # frame 0 that is the entropy of softmax(pi + o_0) at every t
    flat = np.array(obs)
    flat[:, 1:] = np.float32(-1.5)
    H, L, prefix = host64(flat, frames, A, pi)
    x = np.asarray(pi, np.float64) + flat[:, 0].astype(np.float64)
    logp = x - np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)) - x.max(1, keepdims=True)
    first = -(np.exp(logp) * logp).sum(1)
    F = pec.clamp(frames, T)
    for b in range(B):
        pec.close(prefix[b, :F[b]], np.full(F[b], first[b]), pec.reference_bound(first[b]), b)
    one_hot = np.full(S, -np.inf, np.float32)
    one_hot[4] = 0.
    H, L, prefix = host64(obs, frames, A, one_hot)
    assert (H == 0).all() and (prefix == 0).all() and np.isfinite(L).all()


# ------------------------------------------------------------------------------------------------ the uniform collapse
@pytest.mark.parametrize('B,T,S', [(2, 5, 1), (3, 6, 3), (3, 7, 65)])
def test_uniform_route_equals_the_dense_route_on_the_filled_matrix(B, T, S):
    obs, frames, _, pi = pec.softmax_case(B, T, S, 11 * S + T, matrix=None)
    got = host64(obs, frames, None, pi)
    want = host64(obs, frames, pec.filled(S), pi)
    for g, w in zip(got, want):
        pec.close(g, w, pec.reference_bound(w), 'uniform against dense')
    # frames are independent: prefix_t is the running sum of the entropies of softmax(o_s), pi + o_0 at s = 0
    x = obs.astype(np.float64)
    x[:, 0] += pi.astype(np.float64)
    logp = x - np.log(np.exp(x).sum(2, keepdims=True))
    rows = np.cumsum(-(np.exp(logp) * logp).sum(2), axis=1)
    F = pec.clamp(frames, T)
    for b in range(B):
        pec.close(got[2][b, :F[b]], rows[b, :F[b]], pec.reference_bound(rows[b, :F[b]]), b)


# ------------------------------------------------------------------------------------------------ the non-finite rules
@pytest.mark.parametrize('value', [math.nan, math.inf])
@pytest.mark.parametrize('where', ['observation', 'observation_beyond', 'initial', 'matrix', 'uniform_observation',
                                   'uniform_initial'])
def test_non_finite_rule(where, value):
    B, T, S = 4, 5, 7
    uniform = where.startswith('uniform')
    obs, _, A, pi = pec.softmax_case(B, T, S, 21, matrix=None if uniform else 'dense')
    frames = np.array([5, 3, 1, 4], np.int32)
    clean = host64(obs, frames, A, pi)
    obs, pi = np.array(obs), np.array(pi)
    A = None if uniform else np.array(A)
    if where.endswith('observation'):
        obs[1, 2, 4] = value                                     # item 1, inside its 3 frames
        bad = [1]
    elif where == 'observation_beyond':
        obs[1, 3, 4] = value                                     # item 1, behind its frames: nobody reads it
        bad = []
    elif where.endswith('initial'):
        pi[2] = value
        bad = [0, 1, 2, 3]
    else:
        A[3, 1] = value
        bad = [0, 1, 3]                                          # item 2 has one frame and reads no matrix
    H, L, prefix = host64(obs, frames, A, pi)
    for b in range(B):
        f = int(frames[b])
        if b in bad:
            assert np.isnan(H[b]) and np.isnan(L[b]) and np.isnan(prefix[b, :f]).all() and (prefix[b, f:] == 0).all()
        else:                                                    # the neighbours' bits do not change
            assert all(np.array_equal(words(g[b:b + 1]), words(c[b:b + 1])) for g, c in zip((H, L, prefix), clean))


@pytest.mark.parametrize('matrix', ['dense', None])
def test_an_item_of_total_probability_zero(matrix):
    B, T, S = 3, 4, 5
    obs, _, A, pi = pec.softmax_case(B, T, S, 3, matrix=matrix)
    frames = np.array([4, 4, 2], np.int32)
    clean = host64(obs, frames, A, pi)
    obs = np.array(obs)
    obs[1, 2, :] = -np.inf                                       # no state can emit frame 2 of item 1
    H, L, prefix = host64(obs, frames, A, pi)
    assert L[1] == -np.inf and np.isnan(H[1]) and np.isnan(prefix[1]).all()
    for b in (0, 2):
        assert all(np.array_equal(words(g[b:b + 1]), words(c[b:b + 1])) for g, c in zip((H, L, prefix), clean))
    got = entropy.forward_entropy(*pec.tensors(obs, frames, A, pi))
    assert got[1][1] == -math.inf and torch.isnan(got[0][1])


# ------------------------------------------------------------------------------------------------ the front
def test_default_arguments_and_log_probs_both_ways():
    B, T, S = 2, 4, 5
    g = torch.Generator().manual_seed(1)
    p = torch.softmax(torch.randn(B, T, S, generator=g), 2)
    A = torch.softmax(torch.randn(S, S, generator=g), 0)
    pi = torch.softmax(torch.randn(S, generator=g), 0)
    before = p.clone()
    H, L = entropy.path_entropy(p, gpu=None)
    assert H.shape == L.shape == (B,) and H.dtype == L.dtype == torch.float32 and H.device == CPU and torch.equal(p, before)
    log_obs = inputs.observation(p, False, CPU)
    default_pi = torch.full((S,), math.log(1. / S + torch.finfo(torch.float32).tiny), dtype=torch.float32)
    want = entropy.forward_entropy(log_obs, None, None, default_pi, prefix=True)
    got = entropy.path_entropy(p, gpu=None, prefix=True)
    assert len(got) == 3 and got[2].shape == (B, T) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(H, want[0]) and torch.equal(L, want[1])
    ref = pec.loop(log_obs.numpy(), [T] * B, None, default_pi.numpy())
    pec.close(H.numpy(), ref[0], 1e-6 * (1 + np.abs(ref[0])), 'float32 rounding of the float64 value')
    # probabilities and their logarithms name the same model
    plain = entropy.path_entropy(p, torch.tensor([T, 2]), A, pi, gpu=None, prefix=True)
    logs = entropy.path_entropy(torch.log(p), torch.tensor([T, 2]), torch.log(A), torch.log(pi), log_probs=True, gpu=None,
                                prefix=True)
    assert all(torch.equal(a, b) for a, b in zip(plain, logs))
    direct = entropy.forward_entropy(log_obs, torch.tensor([T, 2]), torch.log(A), torch.log(pi), prefix=True)
    assert all(torch.equal(a, b) for a, b in zip(plain, direct)) and (plain[2][1, 2:] == 0).all()


def test_an_empty_batch_and_bad_shapes():
    H, L, prefix = entropy.forward_entropy(torch.empty(0, 3, 4), None, None, torch.zeros(4), prefix=True)
    assert H.shape == L.shape == (0,) and prefix.shape == (0, 3)
    H, L = entropy.path_entropy(torch.empty(0, 3, 4), gpu=None)
    assert H.shape == L.shape == (0,)
    with pytest.raises(RuntimeError, match='initial'):
        entropy.forward_entropy(torch.zeros(1, 2, 3), None, None, None)
    with pytest.raises(RuntimeError, match='transition must have shape'):
        entropy.forward_entropy(torch.zeros(1, 2, 3), None, torch.zeros(2, 2), torch.zeros(3))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_surface():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    declared = set(re.findall(r'\b(torbi_hip_\w+)\s*\(', header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert not name.endswith('_bytes')
    assert _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert 'entropy' in torbi_amd.__all__ and torbi_amd.entropy is entropy
    assert not set(entropy.__all__) & set(torbi_amd.__all__)
    assert all(not hasattr(torbi_amd, name) for name in entropy.__all__)
    size = lib.torbi_hip_path_entropy_workspace_size
    for nonsense in [(0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (-1, 5, 5, 1), (1, 1, 16385, 0), (0, 0, 0, 1)]:
        assert size(*nonsense) == 256, nonsense
    assert entropy.path_entropy_workspace_bytes(3, 7, 65) == size(3, 7, 65, 0)
    assert entropy.path_entropy_workspace_bytes(3, 7, 65, uniform=True) == size(3, 7, 65, 1)


def test_workspace_size_is_its_stated_layout():
    """E and G padded to (S up to 64) x (S up to 32); m, c and prefix [B][T]; the partials and the p and u rows for two
    parities; every piece rounded up to 256 bytes, and 256 to align the base.  No term grows as B T S."""
    size = _lib.load().torbi_hip_path_entropy_workspace_size
    up = lambda n, a: -(-n // a) * a
    for B, T, S in [(1, 1, 1), (3, 7, 65), (17, 5, 1441), (512, 500, 1440), (5, 3, 16384)]:
        Sp, Mp, P = up(S, 32), up(S, 64), -(-S // 32)
        pieces = [Mp * Sp, Mp * Sp, B * T, B * T, 2 * B * P, 2 * B * Sp, 2 * B * Sp, B * T]
        assert size(B, T, S, 0) == sum(up(4 * n, 256) for n in pieces) + 256, (B, T, S)
        assert size(B, T, S, 1) == 2 * up(8 * B * T, 256) + 256, (B, T, S)
    # doubling the frames adds what the [B][T] pieces add, whatever the states
    for S in (65, 1440):
        grown = size(512, 1000, S, 0) - size(512, 500, S, 0)
        assert grown == 3 * 4 * 512 * 500
    assert size(512, 500, 1440, 0) < 512 * 500 * 1440 * 4 // 40


def test_argument_errors_are_answered_before_a_device_is_touched():
    lib = _lib.load()
    B, T, S = 2, 3, 4
    p = np.zeros(64, np.float32).ctypes.data                    # host memory nobody reads
    need = lib.torbi_hip_path_entropy_workspace_size(B, T, S, 0)
    uneed = lib.torbi_hip_path_entropy_workspace_size(B, T, S, 1)

    def dense(obs=p, frames=p, A=p, pi=p, h=p, prefix=p, l=p, ws=p, nbytes=need, B=B, T=T, S=S):
        return lib.torbi_hip_path_entropy(obs, frames, A, pi, h, prefix, l, ws, nbytes, B, T, S, 0, None)

    def uniform(obs=p, frames=p, pi=p, h=p, prefix=p, l=p, ws=p, nbytes=uneed, B=B, T=T, S=S):
        return lib.torbi_hip_path_entropy_uniform(obs, frames, -1.25, pi, h, prefix, l, ws, nbytes, B, T, S, 0, None)

    EINVAL, EWORKSPACE, ERANGE = -1, -2, -3
    for call in (dense, uniform):
        assert call(B=0) == 0 and call(B=0, obs=None, ws=None, nbytes=0) == 0
        for shape in (dict(B=-1), dict(T=0), dict(S=0)):
            assert call(**shape) == EINVAL, shape
        for name in ('obs', 'frames', 'pi', 'h', 'l', 'ws'):
            assert call(**{name: None}) == EINVAL, name
        # the order: EINVAL before ERANGE before EWORKSPACE
        assert call(S=16385, nbytes=1 << 40) == ERANGE and call(S=16385, nbytes=0) == ERANGE
        assert call(S=16385, nbytes=0, obs=None) == EINVAL
        assert call(nbytes=(need if call is dense else uneed) - 1) == EWORKSPACE
        assert call(prefix=None, nbytes=0) == EWORKSPACE           # (a missing prefix output is no error)
    assert dense(A=None) == EINVAL


# ------------------------------------------------------------------------------------------------ operand forms
FORM_CASES = pec.form_cases(CPU)


@pytest.mark.parametrize('name,operand,form_name', FORM_CASES, ids=['-'.join(c) for c in FORM_CASES])
def test_a_form_equals_its_plain_copy_and_nothing_is_written(name, operand, form_name):
    ofc.check_forms(pec.ENTRY[name], CPU, None, {operand: form_name})


@pytest.mark.parametrize('name', list(pec.ENTRY))
def test_every_operand_in_another_form_at_once(name):
    entry = pec.ENTRY[name]
    ofc.check_forms(entry, CPU, None, {operand: ofc.TOGETHER[operand] for operand in entry.operands})
