"""torbi_amd.best_paths / decode_k_best on an MI355X (csrc/k_best.hpp) against the host route, bit for bit; the host route
is checked against brute-force enumeration in tests/test_k_best_cpu.py."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import synth
from k_best_cases import step_items

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def host(obs, frames, trans, init, k):
    t = None if trans is None else torch.as_tensor(trans)
    i, s = torbi_amd.decode_k_best(torch.as_tensor(obs), torch.as_tensor(frames), t, torch.as_tensor(init), k)
    return i.numpy(), s.numpy()


def device(obs, frames, trans, init, k, workspace=None):
    t = None if trans is None else torch.as_tensor(trans).to(DEV)
    i, s = torbi_amd.decode_k_best(torch.as_tensor(obs).to(DEV), torch.as_tensor(frames).to(DEV), t,
                                   torch.as_tensor(init).to(DEV), k, workspace=workspace)
    assert i.device == DEV and i.dtype == torch.int32 and s.dtype == torch.float32
    return i.cpu().numpy(), s.cpu().numpy()


def same(got, want):
    gi, gs = got
    wi, ws = want
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:10]
    assert np.array_equal(gs.view(np.int32), ws.view(np.int32)), (gs, ws)


def ragged(B, T, seed):
    frames = np.clip(synth.lengths(B, 1, T, seed=seed), 1, T).astype(np.int32)
    frames[0] = T
    return frames


def banded(S, tiny):
    return synth.banded_transition(S, max(1.5, S / 16.5), tiny=tiny).astype(np.float32)


# every step instance with more than one item per workgroup; B is not a multiple of G, so the last group has a tail
MULTI = [(4093, 5, 64, 1), (4093, 5, 64, 2), (3001, 5, 64, 1), (3001, 5, 64, 2), (2047, 5, 64, 3), (1500, 5, 64, 1),
         (1500, 5, 64, 2), (1500, 5, 64, 4), (1023, 5, 64, 5)]


def test_multi_item_cases_reach_every_instance():
    built = {(km, g) for km in (1, 2, 4, 8, 16, 32) for g in (2, 4, 8) if g * km <= 16}
    assert {step_items(B, S, k) for (B, T, S, k) in MULTI} == built


@pytest.mark.parametrize('B,T,S,k', MULTI)
@pytest.mark.parametrize('kind', ['dense', 'band_tiny'])
def test_against_host_route_several_items_per_workgroup(B, T, S, k, kind):
    obs, trans, init = synth.problem(B, T, S, seed=B + k)
    if kind == 'band_tiny':
        trans = banded(S, True)
    frames = ragged(B, T, B + k)
    frames[-1] = T
    assert step_items(B, S, k)[1] > 1
    same(device(obs, frames, trans, init, k), host(obs, frames, trans, init, k))


GRID = [(1, 9, 1, 3), (3, 12, 3, 2), (5, 10, 7, 5), (40, 16, 64, 16), (17, 12, 65, 32), (9, 14, 255, 5),
        (200, 6, 64, 2), (6, 9, 360, 16), (16, 10, 1440, 1), (3, 8, 1440, 5), (2, 4, 1440, 16), (2, 3, 1440, 32)]


@pytest.mark.parametrize('B,T,S,k', GRID)
@pytest.mark.parametrize('kind', ['dense', 'band', 'band_tiny', 'uniform'])
def test_against_host_route(B, T, S, k, kind):
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S + k)
    if kind.startswith('band'):
        trans = banded(S, kind == 'band_tiny')
    elif kind == 'uniform':
        trans = None
    frames = ragged(B, T, S + k)
    same(device(obs, frames, trans, init, k), host(obs, frames, trans, init, k))


def test_uniform_route_equals_the_fill_matrix_on_device():
    B, T, S, k = 7, 11, 65, 5
    obs, _, init = synth.problem(B, T, S, seed=3)
    fill = torch.full((S, S), math.log(1. / S), dtype=torch.float32).numpy()
    frames = ragged(B, T, 2)
    same(device(obs, frames, None, init, k), device(obs, frames, fill, init, k))


@pytest.mark.parametrize('B,T,S,k', [(64, 200, 1440, 4), (33, 50, 1440, 1), (20, 40, 255, 7), (512, 6, 1440, 1),
                                   (512, 6, 1440, 4), (509, 6, 1440, 2)])
@pytest.mark.parametrize('kind', ['dense', 'band', 'band_tiny'])
def test_rank_zero_is_the_gpu_decode(B, T, S, k, kind):
    obs, trans, init = synth.problem(B, T, S, seed=11)
    if kind != 'dense':
        trans = banded(S, kind == 'band_tiny')
    frames = ragged(B, T, 5)
    t = torch.as_tensor(obs).to(DEV)
    f = torch.as_tensor(frames).to(DEV)
    A = torch.as_tensor(trans).to(DEV)
    pi = torch.as_tensor(init).to(DEV)
    want = torbi_amd.decode(t, f, A, pi).cpu().numpy()
    i, s = torbi_amd.decode_k_best(t, f, A, pi, k)
    assert np.array_equal(i[:, 0].cpu().numpy(), want)
    assert (s[:, :-1] >= s[:, 1:]).all()


def test_rank_zero_is_from_probabilities_on_device():
    B, T, S, k = 12, 30, 128, 4
    rng = np.random.default_rng(0)
    p = torch.tensor(rng.random((B, T, S), dtype=np.float32))
    p = p / p.sum(-1, keepdim=True)
    A = torch.tensor(rng.random((S, S), dtype=np.float32))
    A = A / A.sum(-1, keepdim=True)
    frames = torch.tensor(ragged(B, T, 9))
    want = torbi_amd.from_probabilities(p, frames, A, gpu=0).cpu()
    i, s = torbi_amd.best_paths(p, k, frames, A, gpu=0)
    assert i.device == DEV
    assert torch.equal(i[:, 0].cpu(), want)
    assert (s[:, :-1] >= s[:, 1:]).all()


def test_nonfinite_items_are_flagged_and_isolated():
    B, T, S, k = 6, 9, 33, 4
    obs, trans, init = synth.problem(B, T, S, seed=21)
    frames = np.array([9, 9, 4, 9, 9, 9], dtype=np.int32)
    obs[1, 3, 5] = np.nan
    obs[2, 6, 0] = np.inf          # beyond its frames: not read
    obs[3, 0, 7] = np.inf
    obs[4, 8, 2] = -np.inf         # a real -inf
    got = device(obs, frames, trans, init, k)
    same(got, host(obs, frames, trans, init, k))
    assert np.isnan(got[1][[1, 3]]).all() and (got[0][[1, 3]] == -1).all()
    assert np.isfinite(got[1][[0, 2, 4, 5]]).all()


@pytest.mark.parametrize('B,T,S,k', [(24, 20, 96, 6), (2047, 12, 64, 4), (4093, 8, 64, 2)])
@pytest.mark.parametrize('trans_kind', ['dense', 'uniform'])
def test_item_independence(B, T, S, k, trans_kind):
    """Items 5 and B - 1 keep their bits when every other item changes, including a NaN item in item 5's workgroup."""
    obs, trans, init = synth.problem(B, T, S, seed=8)
    if trans_kind == 'uniform':
        trans = None
    frames = ragged(B, T, 4)
    a = device(obs, frames, trans, init, k)
    other = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), seed=99)
    keep = [5, B - 1]
    other[keep] = obs[keep]
    other[4, 2, 3] = np.nan
    frames2 = ragged(B, T, 6)
    frames2[keep] = frames[keep]
    frames2[4] = T                     # (so that item 4 reads its NaN)
    b = device(other, frames2, trans, init, k)
    same((b[0][keep], b[1][keep]), (a[0][keep], a[1][keep]))
    assert np.isnan(b[1][4]).all()


@pytest.mark.parametrize('uniform', [False, True])
def test_graph_capture_and_replay(uniform):
    B, T, S, k = 16, 24, 200, 4
    obs, trans, init = synth.problem(B, T, S, seed=31)
    frames = torch.tensor(ragged(B, T, 3), device=DEV)
    A = None if uniform else torch.tensor(trans, device=DEV)
    pi = torch.tensor(init, device=DEV)
    x = torch.tensor(obs, device=DEV)
    ws = torch.empty(torbi_amd.decode_k_best_workspace_bytes(B, T, S, k, uniform=uniform), dtype=torch.uint8, device=DEV)
    torbi_amd.decode_k_best(x, frames, A, pi, k, workspace=ws)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torbi_amd.decode_k_best(x, frames, A, pi, k, workspace=ws)
    for seed in (32, 33):
        x.copy_(torch.tensor(synth.scores(synth.STREAM_OBSERVATION, (B, T, S), seed=seed), device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = torbi_amd.decode_k_best(x, frames, A, pi, k)
        assert torch.equal(out[0], want[0])
        assert torch.equal(out[1].view(torch.int32), want[1].view(torch.int32))
