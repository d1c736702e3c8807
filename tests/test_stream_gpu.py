"""torbi_amd.StreamDecoder through the HIP route (torbi_hip_stream_*): bit-identical to the whole-sequence decode on the
same device and to the oracle, and the same commits as the host decoder push for push."""
import math

import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def peaked(B, T, S, seed=0):
    """Posteriorgram-like log-probabilities: per-frame log_softmax of logits peaked around a moving centre."""
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, T, S), generator=gen) * 2.0
    centre = (S / 2 + torch.cumsum(torch.randn((B, T, 1), generator=gen) * 6, dim=1)).clamp(0, S - 1)
    logits -= ((torch.arange(S)[None, None, :] - centre).abs() / 12.0) ** 2
    return torch.log_softmax(logits, dim=-1).clamp_(min=math.log(torch.finfo(torch.float32).tiny)).numpy()


def run(dec, obs, Tc, lengths=None, ragged=None, host=None):
    """Push obs (B, T, S) (numpy) in pieces of Tc frames (`ragged`: random per-stream counts instead); `host`: a host
    decoder fed the same pieces, whose `pending` must match after every push.  Returns per-stream outputs and lengths."""
    B, T, S = obs.shape
    lengths = np.full(B, T) if lengths is None else lengths
    rng = np.random.default_rng(ragged or 0)
    pos = np.zeros(B, dtype=np.int64)
    got = [[] for _ in range(B)]
    while (pos < lengths).any():
        f = np.minimum(lengths - pos, rng.integers(0, Tc + 1, size=B) if ragged else Tc)
        chunk = np.full((B, Tc, S), np.nan, np.float32)
        for b in range(B):
            chunk[b, :f[b]] = obs[b, pos[b]:pos[b] + f[b]]
        out = dec.push(torch.from_numpy(chunk).to(DEV), torch.from_numpy(f))
        for b in range(B):
            assert out[b].device == DEV and out[b].dtype == torch.int32
            got[b].append(out[b].cpu())
        if host is not None:
            host.push(torch.from_numpy(chunk), torch.from_numpy(f))
            assert torch.equal(dec.pending, host.pending), (dec.pending, host.pending)
        pos += f
    for b, rest in enumerate(dec.flush()):
        got[b].append(rest.cpu())
    return [torch.cat(g).numpy() for g in got], pos


def check(obs, trans, init, Tc, ragged=None, oracle_items=2, log_probs=True, host=False, lengths=None):
    B, T, S = obs.shape
    t = None if trans is None else torch.from_numpy(trans).to(DEV)
    i = None if init is None else torch.from_numpy(init).to(DEV)
    dec = torbi_amd.StreamDecoder(B, S, t, i, log_probs=log_probs, gpu=0)
    twin = None
    if host:
        twin = torbi_amd.StreamDecoder(B, S, None if trans is None else torch.from_numpy(trans),
                                       None if init is None else torch.from_numpy(init), log_probs=log_probs, gpu=None)
    got, n = run(dec, obs, Tc, lengths=lengths, ragged=ragged, host=twin)
    frames = torch.from_numpy(np.maximum(n, 1).astype(np.int32))
    want = torbi_amd.from_probabilities(torch.from_numpy(obs).to(DEV), frames.to(DEV), t, i, log_probs, gpu=0).cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], want[b, :n[b]]), (b, np.flatnonzero(got[b] != want[b, :n[b]])[:10])
    if log_probs and trans is not None:
        x = torch.from_numpy(obs[:oracle_items]).clone()
        torch.exp_(x)
        x += torch.finfo(torch.float32).tiny
        torch.log_(x)
        o = oracle.decode(x.numpy(), n[:oracle_items].astype(np.int32), trans, init, num_threads=oracle.max_threads())
        for b in range(oracle_items):
            assert np.array_equal(got[b], o[b, :n[b]]), b


@pytest.mark.parametrize('Tc', [1, 7, 100])
def test_one_stream_1440(Tc):
    obs, trans, init = synth.problem(1, 500, 1440, seed=1)
    check(obs, trans, init, Tc, oracle_items=1)


def test_batch_512_pushes_of_50():
    obs, trans, init = synth.problem(512, 500, 1440, seed=2)
    check(obs, trans, init, 50, oracle_items=4)


@pytest.mark.parametrize('S', [64, 257, 4096])
def test_state_counts_ragged(S):
    T = 30 if S == 4096 else 80
    obs, trans, init = synth.problem(4, T, S, seed=S)
    check(obs, trans, init, 9, ragged=S, oracle_items=1 if S == 4096 else 4, host=S < 4096)


def test_pitch_band_matrix():
    S = 1440
    obs = peaked(8, 200, S, seed=3)
    trans = synth.banded_transition(S, 87.2)
    init = np.full(S, math.log(1. / S), np.float32)
    check(obs, trans, init, 25, oracle_items=2)
    check(obs[:2], synth.banded_transition(S, 87.2, tiny=True), init, 10, ragged=4, oracle_items=2)


def test_uniform_default_with_probabilities():
    B, T, S = 6, 120, 360
    rng = np.random.default_rng(5)
    p = rng.dirichlet(np.ones(S), size=(B, T)).astype(np.float32)
    check(p, None, None, 16, ragged=5, log_probs=False)


def test_nonfinite_inputs():
    B, T, S = 4, 60, 257
    obs, trans, init = synth.problem(B, T, S, seed=9)
    obs = obs.copy()
    rng = np.random.default_rng(1)
    for value in (np.nan, np.inf, -np.inf):
        obs.reshape(-1)[rng.integers(0, obs.size, size=40)] = value
    obs[1, 10, 0] = np.nan
    obs[3, 20, :] = np.nan
    check(obs, trans, init, 7, ragged=9, oracle_items=4, host=True)
    t2 = trans.copy()
    t2[4, 0] = np.nan
    t2[7, 3] = np.inf
    t2[:, 11] = -np.inf
    check(obs, t2, init, 7, oracle_items=4, host=True)


def test_pending_matches_host_decoder():
    """Maximal commit at a size the numpy brute force of the CPU tests cannot reach: the device decoder's `pending` equals
    the host decoder's after every push, on posteriorgram-like inputs with the pitch matrix."""
    S = 1440
    obs = peaked(3, 60, S, seed=6)
    check(obs, synth.banded_transition(S, 87.2), np.zeros(S, np.float32), 6, ragged=6, oracle_items=1, host=True)


def test_growing_window_identity():
    B, T, S = 2, 2000, 16
    obs, _, init = synth.problem(B, T, S, seed=12)
    ident = np.full((S, S), -np.inf, np.float32)
    np.fill_diagonal(ident, 0.)
    dec = torbi_amd.StreamDecoder(B, S, torch.from_numpy(ident).to(DEV), torch.from_numpy(init).to(DEV), log_probs=True, gpu=0)
    for t in range(0, T, 10):
        out = dec.push(torch.from_numpy(obs[:, t:t + 10]).to(DEV))
        assert all(o.numel() == 0 for o in out)
    assert dec.pending.tolist() == [T] * B
    rest = dec.flush()
    want = torbi_amd.from_probabilities(torch.from_numpy(obs).to(DEV), None, torch.from_numpy(ident).to(DEV),
                                        torch.from_numpy(init).to(DEV), True, gpu=0).cpu().numpy()
    for b in range(B):
        assert np.array_equal(rest[b].cpu().numpy(), want[b])


def test_flush_one_stream_restarts_from_initial():
    B, T, S = 3, 40, 257
    obs, trans, init = synth.problem(B, 2 * T, S, seed=13)
    t, i = torch.from_numpy(trans).to(DEV), torch.from_numpy(init).to(DEV)
    dec = torbi_amd.StreamDecoder(B, S, t, i, log_probs=True, gpu=0)
    got = [[] for _ in range(B)]
    for k in range(0, T, 8):
        for b, o in enumerate(dec.push(torch.from_numpy(obs[:, k:k + 8]).to(DEV))):
            got[b].append(o.cpu())
    got[2] += [r.cpu() for r in dec.flush(items=[2])]
    first = torch.cat(got[2]).numpy()
    got[2] = []
    for k in range(T, 2 * T, 8):
        for b, o in enumerate(dec.push(torch.from_numpy(obs[:, k:k + 8]).to(DEV))):
            got[b].append(o.cpu())
    for b, r in enumerate(dec.flush()):
        got[b].append(r.cpu())

    def whole(x):
        return torbi_amd.from_probabilities(torch.from_numpy(np.ascontiguousarray(x)).to(DEV)[None], None, t, i, True,
                                            gpu=0)[0].cpu().numpy()
    assert np.array_equal(first, whole(obs[2, :T]))
    assert np.array_equal(torch.cat(got[2]).numpy(), whole(obs[2, T:]))
    for b in (0, 1):
        assert np.array_equal(torch.cat(got[b]).numpy(), whole(obs[b]))
