"""torbi_amd.StreamDecoder on the host (gpu=None): exactness against the whole-sequence decode and the oracle, and the
maximal-commit rule against a brute-force survivor-set computation."""
import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth
from stream_cases import plan, feed, clamp, commit_checker


def whole(obs, trans, init, log_probs=True):
    """from_probabilities on one whole sequence (gpu=None)."""
    t = None if trans is None else torch.from_numpy(np.asarray(trans))
    i = None if init is None else torch.from_numpy(np.asarray(init))
    return torbi_amd.from_probabilities(torch.from_numpy(np.ascontiguousarray(obs))[None], None, t, i, log_probs,
                                        gpu=None)[0].numpy()


def check_exact(source, trans, init, pushes, with_oracle=True, log_probs=True):
    B, S = len(source), source[0].shape[1]
    dec = torbi_amd.StreamDecoder(B, S, None if trans is None else torch.from_numpy(trans),
                                  None if init is None else torch.from_numpy(init), log_probs=log_probs, gpu=None)
    got, pos = feed(dec, source, pushes)
    for b in range(B):
        seq = source[b][:pos[b]]
        if pos[b] == 0:
            assert got[b].size == 0
            continue
        want = whole(seq, trans, init, log_probs)
        assert np.array_equal(got[b], want), (b, got[b], want)
        if with_oracle:
            o = oracle.decode(clamp(seq)[None], np.array([len(seq)], np.int32), trans, init)[0]
            assert np.array_equal(got[b], o), (b, got[b], o)
            c = torbi_amd.decode_cpu(torch.from_numpy(clamp(seq)[None]), torch.tensor([len(seq)], dtype=torch.int32),
                                     torch.from_numpy(trans), torch.from_numpy(init))[0].numpy()
            assert np.array_equal(got[b], c)
    return got


@pytest.mark.parametrize('S', [1, 3, 17, 64, 257])
@pytest.mark.parametrize('mode', ['all', 'one', 'random', 'ragged'])
def test_exact_against_whole_sequence_and_oracle(S, mode):
    B, T = 3, (12 if S == 257 else 30)
    obs, trans, init = synth.problem(B, T, S, seed=S)
    check_exact([obs[b] for b in range(B)], trans, init, plan(B, T, mode, seed=S))


def test_readme_toy():
    observation = torch.tensor([[[0.25, 0.5, 0.25], [0.25, 0.25, 0.5], [0.33, 0.33, 0.33]]])
    transition = torch.tensor([[0.5, 0.25, 0.25], [0.33, 0.34, 0.33], [0.25, 0.25, 0.5]])
    initial = torch.tensor([0.4, 0.35, 0.25])
    for Tc in (1, 2, 3):
        dec = torbi_amd.StreamDecoder(1, 3, transition, initial, gpu=None)
        out = []
        for t in range(0, 3, Tc):
            out += dec.push(observation[:, t:t + Tc])[0].tolist()
        out += dec.flush()[0].tolist()
        assert out == [1, 2, 2]


@pytest.mark.parametrize('mode', ['one', 'ragged'])
def test_ties(mode):
    B, T, S = 3, 20, 17
    zeros = np.zeros((T, S), np.float32)
    check_exact([zeros] * B, np.zeros((S, S), np.float32), np.zeros(S, np.float32), plan(B, T, mode))
    # equal maxima crafted: two states of every row share the largest score
    rng = np.random.default_rng(3)
    obs = np.round(rng.uniform(-3, 0, size=(B, T, S)) * 2).astype(np.float32) / 2
    trans = np.round(rng.uniform(-3, 0, size=(S, S)) * 2).astype(np.float32) / 2
    check_exact([obs[b] for b in range(B)], trans, np.zeros(S, np.float32), plan(B, T, mode, seed=4))


@pytest.mark.parametrize('tiny', [False, True])
@pytest.mark.parametrize('mode', ['one', 'random', 'ragged'])
def test_banded_matrices(tiny, mode):
    B, T, S = 3, 40, 64
    obs, _, init = synth.problem(B, T, S, seed=11)
    trans = synth.banded_transition(S, 5, tiny=tiny)
    check_exact([obs[b] for b in range(B)], trans, init, plan(B, T, mode, seed=5))
    # a narrow -inf band with zero scores elsewhere
    band = np.full((S, S), -np.inf, np.float32)
    for j in range(S):
        band[j, max(0, j - 1):j + 2] = 0.
    check_exact([obs[b] for b in range(B)], band, init, plan(B, T, mode, seed=6))


@pytest.mark.parametrize('mode', ['one', 'random'])
def test_nonfinite_inputs(mode):
    B, T, S = 4, 30, 17
    obs, trans, init = synth.problem(B, T, S, seed=21)
    obs = obs.copy()
    rng = np.random.default_rng(0)
    for value in (np.nan, np.inf, -np.inf):
        idx = rng.integers(0, obs.size, size=12)
        obs.reshape(-1)[idx] = value
    obs[1, 5, 0] = np.nan                       # a NaN at state 0: the reference keeps it
    obs[2, :, :] = -np.inf                      # a whole stream of -inf
    obs[3, 7, :] = np.nan                       # a whole row of NaN
    check_exact([obs[b] for b in range(B)], trans, init, plan(B, T, mode, seed=7))
    t2 = trans.copy()
    t2[3, 0] = np.nan
    t2[5, 2] = np.inf
    t2[:, 9] = -np.inf
    check_exact([obs[b] for b in range(B)], t2, init, plan(B, T, mode, seed=8))


@pytest.mark.parametrize('default', [False, True])
def test_probabilities_in(default):
    B, T, S = 3, 25, 17
    rng = np.random.default_rng(9)
    p = rng.dirichlet(np.ones(S), size=(B, T)).astype(np.float32)
    trans = None if default else rng.dirichlet(np.ones(S), size=S).astype(np.float32)
    init = None if default else rng.dirichlet(np.ones(S)).astype(np.float32)
    check_exact([p[b] for b in range(B)], trans, init, plan(B, T, 'ragged', seed=10), with_oracle=False, log_probs=False)


# ---------------------------------------------------------------------------------------------- maximal commit
@pytest.mark.parametrize('S', [1, 3, 17, 64])
@pytest.mark.parametrize('mode', ['one', 'ragged'])
def test_maximal_commit(S, mode):
    B, T = 3, 40
    obs, trans, init = synth.problem(B, T, S, seed=30 + S)
    source = [obs[b] for b in range(B)]
    dec = torbi_amd.StreamDecoder(B, S, torch.from_numpy(trans), torch.from_numpy(init), log_probs=True, gpu=None)
    feed(dec, source, plan(B, T, mode, seed=S), check=commit_checker(source, trans, init))
    band = synth.banded_transition(S, 3) if S > 3 else trans
    dec = torbi_amd.StreamDecoder(B, S, torch.from_numpy(band), torch.from_numpy(init), log_probs=True, gpu=None)
    feed(dec, source, plan(B, T, mode, seed=S), check=commit_checker(source, band, init))


def test_uniform_transition_leaves_one_pending():
    B, T, S = 2, 20, 17
    obs, _, _ = synth.problem(B, T, S, seed=40)
    dec = torbi_amd.StreamDecoder(B, S, log_probs=True, gpu=None)
    for t in range(T):
        dec.push(torch.from_numpy(obs[:, t:t + 1]))
        assert dec.pending.tolist() == [1] * B


def test_identity_never_commits():
    B, T, S = 2, 30, 5
    obs, _, init = synth.problem(B, T, S, seed=41)
    ident = np.full((S, S), -np.inf, np.float32)
    np.fill_diagonal(ident, 0.)
    dec = torbi_amd.StreamDecoder(B, S, torch.from_numpy(ident), torch.from_numpy(init), log_probs=True, gpu=None)
    for t in range(0, T, 3):
        out = dec.push(torch.from_numpy(obs[:, t:t + 3]))
        assert all(o.numel() == 0 for o in out)
    rest = dec.flush()
    for b in range(B):
        assert np.array_equal(rest[b].numpy(), whole(obs[b], ident, init))


def test_flush_one_stream_and_restart():
    B, T, S = 3, 24, 17
    obs, trans, init = synth.problem(B, 2 * T, S, seed=50)
    dec = torbi_amd.StreamDecoder(B, S, torch.from_numpy(trans), torch.from_numpy(init), log_probs=True, gpu=None)
    got = [[] for _ in range(B)]
    for t in range(0, T, 4):
        for b, o in enumerate(dec.push(torch.from_numpy(obs[:, t:t + 4]))):
            got[b].append(o)
    got[1] += dec.flush(items=[1])
    assert int(dec.frames[1]) == 0 and int(dec.pending[1]) == 0 and int(dec.frames[0]) == T
    first = torch.cat(got[1]).numpy()
    assert np.array_equal(first, whole(obs[1, :T], trans, init))
    got[1] = []
    for t in range(T, 2 * T, 4):          # stream 1 starts a new sequence from `initial`; 0 and 2 go on
        for b, o in enumerate(dec.push(torch.from_numpy(obs[:, t:t + 4]))):
            got[b].append(o)
    for b, rest in enumerate(dec.flush()):
        got[b].append(rest)
    assert np.array_equal(torch.cat(got[0]).numpy(), whole(obs[0], trans, init))
    assert np.array_equal(torch.cat(got[2]).numpy(), whole(obs[2], trans, init))
    assert np.array_equal(torch.cat(got[1]).numpy(), whole(obs[1, T:], trans, init))
    assert all(r.numel() == 0 for r in dec.flush())          # nothing left after a flush
    # a stream flushed after one frame returns the argmax of obs[0] + initial
    dec.push(torch.from_numpy(obs[:, :1]))
    assert dec.flush(items=[2])[0].tolist() == whole(obs[2, :1], trans, init).tolist()


def test_arguments_are_checked():
    dec = torbi_amd.StreamDecoder(2, 3, gpu=None)
    with pytest.raises(ValueError):
        dec.push(torch.zeros(3, 1, 3))
    with pytest.raises(ValueError):
        dec.push(torch.zeros(2, 2, 3), torch.tensor([3, 0]))
    with pytest.raises(IndexError):
        dec.flush(items=[2])
    obs = torch.rand(2, 4, 3)
    kept = obs.clone()
    dec.push(obs)
    assert torch.equal(obs, kept)          # the caller's tensor is not written
