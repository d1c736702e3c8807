"""Max-marginals without a device (torbi_amd/margins.py, MARGINALS.md): the host route against brute-force enumeration on
dyadic inputs and against the numpy loop of the contract bit for bit, the uniform collapse, the score of `best_paths`, the
path of `from_probabilities`, the non-finite rule, the defaults, the C-ABI surface and the operand forms.  The references
and generators are tests/max_marginal_cases.py's; tests/test_max_marginals_gpu.py runs the device route against the same."""
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, inputs, margins

import max_marginal_cases as mmc
import operand_form_cases as ofc

CPU = torch.device('cpu')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('torbi_hip_max_marginals_workspace_size', 'torbi_hip_max_marginals', 'torbi_hip_max_marginals_uniform')


def host(obs, frames, A, pi):
    return margins.forward_backward_max(*mmc.tensors(obs, frames, A, pi))


def words(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32)


# ------------------------------------------------------------------------------------------------ against brute force
@pytest.mark.parametrize('S,T,holes', mmc.DYADIC, ids=[f'S{S}-T{T}-holes{holes}' for S, T, holes in mmc.DYADIC])
def test_host_route_equals_the_enumeration_of_every_path(S, T, holes):
    obs, frames, A, pi, want = mmc.dyadic_case(mmc.DYADIC_ITEMS, T, S, 100 * S + T, holes)
    assert frames[0] == T and frames[-1] == 1                   # ragged, F = 1 included
    got = host(obs, frames, A, pi)
    mmc.same(got, want, (S, T, holes))
    mmc.check_path_consistency(got, frames, (S, T, holes))
    assert not torch.isnan(got[0]).any()
    if holes and S > 1:
        assert np.isneginf(np.asarray(A)).any()
    mmc.same(mmc.loop(obs, frames, A, pi), want, 'the numpy loop itself')


def test_a_state_no_path_reaches_or_leaves_is_minus_inf_not_nan():
    obs, A, pi = mmc.dyadic(2, 4, 3, seed=5)
    A[:, 2] = mmc.NINF                                           # nothing leaves state 2
    A[1, :] = mmc.NINF                                           # nothing reaches state 1
    frames = np.array([4, 3], np.int32)
    m, score = host(obs, frames, A, pi)
    mmc.same((m, score), mmc.brute(obs, frames, A, pi))
    assert not torch.isnan(m).any() and torch.isfinite(score).all()
    assert (m[0, :3, 2] == -math.inf).all() and (m[0, 1:, 1] == -math.inf).all() and (m[0, 3, 2] > -math.inf)


# ------------------------------------------------------------------------------------------------ against the numpy loop
@pytest.mark.parametrize('scale', [.1, 3., 30.])
@pytest.mark.parametrize('B,T,S', [(1, 1, 1), (3, 6, 3), (5, 7, 65), (4, 3, 130)])
def test_host_route_equals_the_numpy_loop_bit_for_bit(B, T, S, scale):
    obs, frames, A, pi, want = mmc.softmax_case(B, T, S, 7 * S + T, scale)
    got = host(obs, frames, A, pi)
    mmc.same(got, want)
    assert np.array_equal(words(got[0]), words(want[0])) and np.array_equal(words(got[1]), words(want[1]))


def test_host_chunks_give_the_same_values(monkeypatch):
    obs, frames, A, pi, want = mmc.softmax_case(5, 7, 65, 7 * 65 + 7, 3.)
    monkeypatch.setattr(margins, '_HOST_CHUNK_ELEMENTS', 65 * 3)              # three rows of one item per chunk
    mmc.same(host(obs, frames, A, pi), want)


@pytest.mark.parametrize('B,T,S', [(1, 1, 1), (2, 5, 1), (3, 6, 3), (5, 7, 65)])
def test_uniform_equals_the_filled_matrix(B, T, S):
    obs, frames, _, pi, want = mmc.softmax_case(B, T, S, 11 * S + T, 3., matrix=False)
    filled = np.full((S, S), mmc.uniform_value(S), np.float32)
    mmc.same(host(obs, frames, None, pi), want, 'uniform against the loop on the filled matrix')
    mmc.same(host(obs, frames, None, pi), [x.numpy() for x in host(obs, frames, filled, pi)], 'uniform against dense')


def test_uniform_equals_the_enumeration_on_dyadic_inputs():
    obs, _, pi = mmc.dyadic(3, 4, 2, seed=9)
    frames = mmc.ragged(3, 4, 9)
    A = np.full((2, 2), -0.75, np.float32)                       # (a dyadic uniform value keeps every sum exact)
    m, score = margins._host(*mmc.tensors(obs, frames), None, -0.75, torch.from_numpy(pi))
    mmc.same((m, score), mmc.brute(obs, frames, A, pi))


# ------------------------------------------------------------------------------------------------ against the decoders
@pytest.mark.parametrize('matrix', [True, False])
def test_score_is_best_paths_score(matrix):
    B, T, S = 4, 6, 9
    g = torch.Generator().manual_seed(3)
    obs = torch.softmax(3 * torch.randn(B, T, S, generator=g), 2)
    A = torch.softmax(torch.randn(S, S, generator=g), 0) if matrix else None
    pi = torch.softmax(torch.randn(S, generator=g), 0)
    frames = torch.from_numpy(mmc.ragged(B, T, 3))
    m, score = margins.max_marginals(obs, frames, A, pi, gpu=None)
    _, want = torbi_amd.best_paths(obs, 1, frames, A, pi, gpu=None)
    assert np.array_equal(words(score), words(want[:, 0]))
    last = m[torch.arange(B), frames.long() - 1]
    assert torch.equal(last.amax(1), score)                      # m_{F-1} is alpha_{F-1} in value


def test_argmax_is_the_decoded_path_where_the_best_path_is_unique():
    found = 0
    for seed in range(40):
        obs, A, pi = mmc.dyadic(3, 5, 3, seed=1000 + seed)
        frames = mmc.ragged(3, 5, seed)
        _, _, best = mmc.brute(obs, frames, A, pi)
        if not (best == 1).all():                                # the case checks itself: one best path, 1/8 above the next
            continue
        found += 1
        ops = mmc.tensors(obs, frames, A, pi)
        m, _ = margins.max_marginals(ops[0], ops[1], ops[2], ops[3], log_probs=True, gpu=None)
        path = torbi_amd.from_probabilities(ops[0], ops[1], ops[2], ops[3], log_probs=True, gpu=None)
        for b in range(3):
            f = int(frames[b])
            assert torch.equal(m[b, :f].argmax(1), path[b, :f].long()), (seed, b)
    assert found >= 5


# ------------------------------------------------------------------------------------------------ NaN and +inf
@pytest.mark.parametrize('value', [math.nan, math.inf])
@pytest.mark.parametrize('where', ['observation', 'observation_beyond', 'initial', 'matrix'])
def test_non_finite_rule(where, value):
    B, T, S = 4, 5, 6
    obs, _, A, pi, clean = mmc.softmax_case(B, T, S, 21)
    frames = np.array([5, 3, 1, 4], np.int32)
    clean = mmc.loop(obs, frames, A, pi)
    obs, A, pi = np.array(obs), np.array(A), np.array(pi)
    if where == 'observation':
        obs[1, 2, 4] = value                                     # item 1, inside its 3 frames
        bad = [1]
    elif where == 'observation_beyond':
        obs[1, 3, 4] = value                                     # item 1, behind its frames: nobody reads it
        bad = []
    elif where == 'initial':
        pi[2] = value
        bad = [0, 1, 2, 3]
    else:
        A[3, 1] = value
        bad = [0, 1, 3]                                          # item 2 has one frame and reads no matrix
    m, score = (x.numpy() for x in host(obs, frames, A, pi))
    mmc.same((m, score), mmc.loop(obs, frames, A, pi), where)
    for b in range(B):
        f = int(frames[b])
        if b in bad:
            assert np.isnan(m[b, :f]).all() and np.isnan(score[b]) and (m[b, f:] == -np.inf).all()
        else:                                                    # the neighbours' values do not change
            assert np.array_equal(words(m[b]), words(clean[0][b])) and words(score)[b] == words(clean[1])[b]


# ------------------------------------------------------------------------------------------------ the front
def test_default_arguments():
    B, T, S = 2, 4, 5
    p = torch.softmax(torch.randn(B, T, S, generator=torch.Generator().manual_seed(1)), 2)
    before = p.clone()
    m, score = margins.max_marginals(p)
    assert m.shape == (B, T, S) and score.shape == (B,) and m.dtype == score.dtype == torch.float32 and m.device == CPU
    assert torch.equal(p, before)
    log_obs = inputs.observation(p, False, CPU)
    pi = torch.full((S,), math.log(1. / S + torch.finfo(torch.float32).tiny), dtype=torch.float32)
    want = margins.forward_backward_max(log_obs, None, None, pi)
    assert torch.equal(m, want[0]) and torch.equal(score, want[1])
    mmc.same((m, score), mmc.loop(log_obs.numpy(), [T] * B, None, pi.numpy()))
    again = margins.max_marginals(torch.log(p), log_probs=True, batch_frames=torch.tensor([T, T]))
    assert torch.equal(again[0], m)


def test_an_empty_batch_and_bad_shapes():
    m, score = margins.forward_backward_max(torch.empty(0, 3, 4), None, None, torch.zeros(4))
    assert m.shape == (0, 3, 4) and score.shape == (0,)
    m, score = margins.max_marginals(torch.empty(0, 3, 4))
    assert m.shape == (0, 3, 4) and score.shape == (0,)
    with pytest.raises(RuntimeError, match='initial'):
        margins.forward_backward_max(torch.zeros(1, 2, 3), None, None, None)
    with pytest.raises(RuntimeError, match='transition must have shape'):
        margins.forward_backward_max(torch.zeros(1, 2, 3), None, torch.zeros(2, 2), torch.zeros(3))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_surface():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    declared = set(re.findall(r'\b(torbi_hip_\w+)\s*\(', header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert not name.endswith('_bytes')
    assert _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert 'margins' in torbi_amd.__all__ and torbi_amd.margins is margins
    assert not set(margins.__all__) & set(torbi_amd.__all__)
    size = lib.torbi_hip_max_marginals_workspace_size
    for nonsense in [(0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (-1, 5, 5, 1), (1, 1, 16385, 0), (0, 0, 0, 1)]:
        assert size(*nonsense) == 256, nonsense
    for uniform in (0, 1):
        by_items = [size(B, 7, 65, uniform) for B in (1, 2, 3, 64, 65, 512)]
        by_states = [size(3, 7, S, uniform) for S in (1, 2, 63, 64, 65, 1440, 4096, 16384)]
        assert by_items == sorted(by_items) and by_states == sorted(by_states) and by_items[0] > 256
        assert all(n % 256 == 0 for n in by_items + by_states)
    assert by_items[-1] > by_items[0]
    # no (B, T, S) region: the matrix, two rows per item and the alarm words, each rounded up to 256 bytes
    assert size(512, 500, 1440, 0) <= 4 * (1440 * 1440 + 2 * 512 * 1440 + 513) + 4 * 256
    assert size(512, 500, 1440, 1) <= 4 * (3 * 512 * 500 + 513) + 5 * 256
    assert margins.max_marginals_workspace_bytes(3, 7, 65) == size(3, 7, 65, 0)
    assert margins.max_marginals_workspace_bytes(3, 7, 65, uniform=True) == size(3, 7, 65, 1)


def test_argument_errors_are_answered_before_a_device_is_touched():
    lib = _lib.load()
    B, T, S = 2, 3, 4
    p = np.zeros(64, np.float32).ctypes.data                    # host memory nobody reads
    need = lib.torbi_hip_max_marginals_workspace_size(B, T, S, 0)
    uneed = lib.torbi_hip_max_marginals_workspace_size(B, T, S, 1)

    def dense(obs=p, frames=p, A=p, pi=p, m=p, s=p, ws=p, nbytes=need, B=B, T=T, S=S):
        return lib.torbi_hip_max_marginals(obs, frames, A, pi, m, s, ws, nbytes, B, T, S, 0, None)

    def uniform(obs=p, frames=p, pi=p, m=p, s=p, ws=p, nbytes=uneed, B=B, T=T, S=S):
        return lib.torbi_hip_max_marginals_uniform(obs, frames, -1.25, pi, m, s, ws, nbytes, B, T, S, 0, None)

    EINVAL, EWORKSPACE, ERANGE = -1, -2, -3
    for call in (dense, uniform):
        assert call(B=0) == 0 and call(B=0, obs=None, ws=None, nbytes=0) == 0
        for shape in (dict(B=-1), dict(T=0), dict(S=0)):
            assert call(**shape) == EINVAL, shape
        for name in ('obs', 'frames', 'pi', 'm', 's', 'ws'):
            assert call(**{name: None}) == EINVAL, name
        assert call(S=16385, nbytes=1 << 40) == ERANGE
        assert call(nbytes=(need if call is dense else uneed) - 1) == EWORKSPACE
    assert dense(A=None) == EINVAL


# ------------------------------------------------------------------------------------------------ operand forms
FORM_CASES = mmc.form_cases(CPU)


@pytest.mark.parametrize('name,operand,form_name', FORM_CASES, ids=['-'.join(c) for c in FORM_CASES])
def test_a_form_equals_its_plain_copy_and_nothing_is_written(name, operand, form_name):
    ofc.check_forms(mmc.ENTRY[name], CPU, None, {operand: form_name})


@pytest.mark.parametrize('name', list(mmc.ENTRY))
def test_every_operand_in_another_form_at_once(name):
    entry = mmc.ENTRY[name]
    ofc.check_forms(entry, CPU, None, {operand: ofc.TOGETHER[operand] for operand in entry.operands})
