"""The band route of k-best decoding on an MI355X (csrc/k_best_band.hpp): `decode_k_best_banded` with the stated band (and
`route='band'` where `viterbi.band_over` is asserted to report that band) against `route='dense'` and the host route, bit
for bit.  The rule itself is checked without a device in tests/test_k_best_band_cpu.py."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import synth
import k_best_band_cases as bc

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def host(obs, frames, trans, init, k):
    i, s = torbi_amd.decode_k_best(torch.as_tensor(obs), torch.as_tensor(frames), torch.as_tensor(trans), torch.as_tensor(init), k)
    return i.numpy(), s.numpy()


def device(obs, frames, trans, init, k, route, workspace=None):
    i, s = torbi_amd.decode_k_best(torch.as_tensor(obs).to(DEV), torch.as_tensor(frames).to(DEV), torch.as_tensor(trans).to(DEV),
                                   torch.as_tensor(init).to(DEV), k, workspace=workspace, route=route)
    assert i.device == DEV and i.dtype == torch.int32 and s.dtype == torch.float32
    return i.cpu().numpy(), s.cpu().numpy()


def same(got, want):
    gi, gs = got
    wi, ws = want
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:10]
    assert np.array_equal(gs.view(np.int32), ws.view(np.int32)), (gs, ws)


def banded(obs, frames, trans, init, k, reach, background):
    """`decode_k_best_banded` with the band as stated: the device runs exactly this reach and this background."""
    i, s = torbi_amd.decode_k_best_banded(torch.as_tensor(obs).to(DEV), torch.as_tensor(frames).to(DEV),
                                          torch.as_tensor(trans).to(DEV), torch.as_tensor(init).to(DEV), k, reach[0], reach[1],
                                          background)
    assert i.device == DEV and i.dtype == torch.int32 and s.dtype == torch.float32
    return i.cpu().numpy(), s.cpu().numpy()


def all_three(obs, frames, trans, init, k, reach, background):
    """band == dense == host, the band route run with the STATED reach and background (`bc.banded` makes the promise hold;
    `route='band'` would take whatever band `viterbi.band_over` reports, which for a finite background is the whole matrix
    as soon as an in-band entry lies below it)."""
    B, T, S = obs.shape
    assert bc.covered(S, k, reach[0], reach[1], background)
    got = banded(obs, frames, trans, init, k, reach, background)
    same(got, device(obs, frames, trans, init, k, 'dense'))
    same(got, host(obs, frames, trans, init, k))
    return got


def known_band(trans, S):
    """What `route='band'` will run for this matrix."""
    A = torch.as_tensor(trans).to(DEV)
    return torbi_amd.viterbi.band_over(A, A, S)


def ragged(B, T, seed):
    frames = np.clip(synth.lengths(B, 1, T, seed=seed), 1, T).astype(np.int32)
    frames[0] = T
    frames[B - 1] = 1
    return frames


def pitch(S, tiny):
    return synth.banded_transition(S, 87.2, tiny=tiny).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1: shapes and bands
@pytest.mark.parametrize('reach', bc.REACHES, ids=lambda r: f'{r[0]}-{r[1]}')
@pytest.mark.parametrize('S', [64, 68, 252, 256, 260])
def test_shapes_reaches_and_backgrounds(S, reach):
    """One wave, a partial second wave, the last lanes of four waves idle, whole waves, a fifth wave of four lanes; every
    reach with every background; k by turns."""
    B, T = 3, 6
    for n, background in enumerate(bc.BACKGROUNDS):
        k = [1, 2, 3, 4, 8, 5][(n + S // 4 + reach[0]) % 6]
        obs, trans, init = bc.model(B, T, S, S + n, reach, background)
        all_three(obs, np.array([T, 1, 4], dtype=np.int32), trans, init, k, reach, background)


# every instance with more than one item per workgroup, B not a multiple of G; the one-item instances beside them
INSTANCES = [(1023, 1), (1023, 2), (1023, 3), (511, 1), (511, 2), (511, 4), (1023, 8), (5, 1), (5, 2), (5, 4), (5, 7), (5, 16),
             (5, 32)]


def test_instance_cases_reach_every_instance():
    built = {(km, g) for km in (1, 2, 4, 8, 16, 32) for g in (1, 2, 4) if g == 1 or g * km <= 16}
    assert {bc.instance(B, 64, k, 5, 2) for B, k in INSTANCES} == built
    for B, k in INSTANCES:
        G = bc.instance(B, 64, k, 5, 2)[1]
        assert G == 1 or B % G != 0


@pytest.mark.parametrize('B,k', INSTANCES)
def test_every_instance_with_a_partial_last_workgroup(B, k):
    T, S, reach, background = 3, 64, (5, 2), -20.         # frame 1 reads lists of one entry, frame 2 full ones
    obs, trans, init = bc.model(B, T, S, 40 + k, reach, background, levels=96)
    all_three(obs, ragged(B, T, 2), trans, init, k, reach, background)


def test_one_frame_and_ragged_frames_from_one():
    S, reach, k = 68, (2, 2), 4
    obs, trans, init = bc.model(5, 1, S, 1, reach, -math.inf)
    got = all_three(obs, np.array([1, 1, 1, 1, 1], dtype=np.int32), trans, init, k, reach, -math.inf)
    assert np.isfinite(got[1]).all()
    obs, trans, init = bc.model(6, 12, S, 2, reach, bc.TINY)
    all_three(obs, np.array([12, 1, 2, 3, 7, 11], dtype=np.int32), trans, init, k, reach, bc.TINY)


@pytest.mark.parametrize('reach', [(0, 0), (0, 3), (3, 0), (2, 2)], ids=lambda r: f'{r[0]}-{r[1]}')
@pytest.mark.parametrize('background', bc.BACKGROUNDS, ids=['inf', 'tiny', 'm20'])
def test_lists_that_grow_over_several_frames(reach, background):
    """Fewer than k in-band candidates in the first frames: with -inf outside, the lists hold -inf entries that point at the
    first pairs (i, r) over ALL prev-states until enough real paths exist."""
    B, T, S, k = 3, 12, 64, 8
    obs, trans, init = bc.model(B, T, S, 9, reach, background)
    all_three(obs, np.array([12, 2, 5], dtype=np.int32), trans, init, k, reach, background)


# ------------------------------------------------------------------------------------------------ 2: ties and -inf
@pytest.mark.parametrize('reach,background,k,levels,dead', bc.BOTH, ids=bc.BOTH_IDS)
def test_tie_and_inf_grids_take_both_paths(reach, background, k, levels, dead):
    obs, frames, trans, init = bc.both_problem(reach, background, levels, dead)
    want = bc.restate(obs, frames, trans, init, k, reach[0], reach[1], background)
    fast, fallback = bc.shares(want[2])
    assert 0 < fallback / (fast + fallback) < 1
    assert want[3].any()                                   # a full in-band list whose k-th value equals dmax
    same(all_three(obs, frames, trans, init, k, reach, background), want[:2])


@pytest.mark.parametrize('k', [1, 2, 4])
def test_an_equal_candidate_left_of_the_band_wins(k):
    """A full in-band list whose k-th value EQUALS dmax, the equal candidates out of band at lower prev-states: a kernel
    with '>=' in place of '>' would return paths from 38 .. 41 (asserted on the restatement in the CPU tests)."""
    obs, frames, trans, init, reach, background = bc.tie_left_of_band(k)
    got = all_three(obs, frames, trans, init, k, reach, background)
    assert (got[0][:, :, 1] == 40).all() and (got[0][:, :, 0] == np.arange(k)).all()


def test_nan_and_all_inf_items_beside_clean_items_of_a_workgroup():
    B, T, S, k, reach, background = 511, 5, 64, 2, (5, 2), -20.
    assert bc.instance(B, S, k, *reach) == (2, 2)
    obs, trans, init = bc.model(B, T, S, 5, reach, background, levels=96)
    frames = np.full(B, T, dtype=np.int32)
    obs[4, 2, 7] = np.nan                 # beside item 5
    obs[6] = -np.inf                      # beside item 7
    obs[9, 4, 1] = np.inf                 # beside item 8
    frames[10] = 3
    obs[10, 3, 0] = np.nan                # beyond its frames: not read
    clean = all_three(np.where(np.isfinite(obs), obs, np.float32(-1.)), frames, trans, init, k, reach, background)
    got = all_three(obs, frames, trans, init, k, reach, background)
    assert np.isnan(got[1][[4, 9]]).all() and (got[0][[4, 9]] == -1).all()
    assert np.isneginf(got[1][6]).all() and (got[0][6] >= 0).all()
    keep = [5, 7, 8, 11, B - 1]
    same((got[0][keep], got[1][keep]), (clean[0][keep], clean[1][keep]))
    assert np.isfinite(got[1][10]).all()


@pytest.mark.parametrize('value', [np.nan, np.inf], ids=['nan', 'plus_inf'])
@pytest.mark.parametrize('background', [-math.inf, -20.], ids=['inf', 'm20'])
def test_nan_or_plus_inf_in_the_matrix_inside_the_band(background, value):
    """The matrix flag of the band route's prepare launch: the promise holds, and the lists are the dense route's and the
    host's (an item of one frame reads no matrix and keeps its scores)."""
    B, T, S, k, reach = 5, 4, 64, 2, (2, 2)
    obs, trans, init = bc.model(B, T, S, 12, reach, background)
    trans[10, 11] = value
    frames = ragged(B, T, 3)
    got = all_three(obs, frames, trans, init, k, reach, background)
    assert np.isnan(got[1][0]).all() and (got[0][0] == -1).all()           # T frames
    assert np.isfinite(got[1][B - 1, 0]) and got[0][B - 1, 0, 0] >= 0         # one frame


@pytest.mark.parametrize('tiny', [False, True], ids=['inf', 'tiny'])
def test_k_one_is_decode(tiny):
    B, T, S = 7, 12, 1440
    obs, _, init = synth.problem(B, T, S, seed=11)
    x, f = torch.as_tensor(obs).to(DEV), torch.as_tensor(ragged(B, T, 5)).to(DEV)
    A, pi = torch.as_tensor(pitch(S, tiny)).to(DEV), torch.as_tensor(init).to(DEV)
    assert torbi_amd.viterbi.band_over(A, A, S) == (87, 87, bc.TINY if tiny else -math.inf)
    i, s = torbi_amd.decode_k_best(x, f, A, pi, 1, route='band')
    assert torch.equal(i[:, 0], torbi_amd.decode(x, f, A, pi))


# ------------------------------------------------------------------------------------------------ 3: the pitch band
@pytest.mark.parametrize('k', [4, 12])
@pytest.mark.parametrize('tiny', [False, True], ids=['inf', 'tiny'])
def test_pitch_band(tiny, k):
    """1440 states, 175 diagonals; k = 12 is the largest the route covers there."""
    B, T, S = 3, 5, 1440
    assert bc.covered(S, 12, 87, 87) and not bc.covered(S, 13, 87, 87)
    # ('auto' takes 175 diagonals up to k = 4, where the probe measured the band route faster: KBEST.md)
    assert torbi_amd.k_best_route(torch.as_tensor(pitch(S, tiny)), B, T, S, k, gpu=0, log_probs=True) == ('band' if k <= 4 else 'dense')
    obs, _, init = synth.problem(B, T, S, seed=3)
    background = bc.TINY if tiny else -math.inf
    frames = np.array([5, 2, 4], dtype=np.int32)
    got = all_three(obs, frames, pitch(S, tiny), init, k, (87, 87), background)
    # `route='band'` finds that band itself
    assert known_band(pitch(S, tiny), S) == (87, 87, background)
    same(device(obs, frames, pitch(S, tiny), init, k, 'band'), got)


# ------------------------------------------------------------------------------------------------ 4: promise and routing
def test_stray_entry_outside_a_stated_band():
    B, T, S, k, reach = 4, 5, 64, 3, (2, 2)
    obs, trans, init = bc.model(B, T, S, 6, reach, -math.inf)
    x, pi = torch.as_tensor(obs).to(DEV), torch.as_tensor(init).to(DEV)
    f = torch.tensor([5, 1, 3, 5], dtype=torch.int32, device=DEV)
    good = torbi_amd.decode_k_best_banded(x, f, torch.as_tensor(trans).to(DEV), pi, k, 2, 2, -math.inf)
    same((good[0].cpu().numpy(), good[1].cpu().numpy()), host(obs, f.cpu().numpy(), trans, init, k))
    trans[40, 37] = -3.                    # one diagonal left of the band
    A = torch.as_tensor(trans).to(DEV)
    i, s = torbi_amd.decode_k_best_banded(x, f, A, pi, k, 2, 2, -math.inf)
    assert torch.isnan(s).all() and (i == -1).all()
    # 'auto' finds the band one diagonal wider and stays exact
    assert torbi_amd.k_best_route(A, B, T, S, k, gpu=0, log_probs=True) == 'band'
    assert torbi_amd.viterbi.band_over(A, A, S) == (3, 2, -math.inf)
    got = torbi_amd.decode_k_best(x, f, A, pi, k, route='auto')
    same((got[0].cpu().numpy(), got[1].cpu().numpy()), host(obs, f.cpu().numpy(), trans, init, k))
    same(device(obs, f.cpu().numpy(), trans, init, k, 'band'), host(obs, f.cpu().numpy(), trans, init, k))


def test_band_raises_where_the_route_does_not_cover():
    S, k = 1440, 4
    obs, trans, init = synth.problem(1, 2, S, seed=1)              # a dense matrix: wider than any band band_over answers for
    args = [torch.as_tensor(a).to(DEV) for a in (obs, np.array([2], dtype=np.int32), trans, init)]
    with pytest.raises(RuntimeError, match='band_over'):
        torbi_amd.decode_k_best(*args, k, route='band')
    assert torbi_amd.k_best_route(args[2], 1, 2, S, k, gpu=0, log_probs=True) == 'dense'
    got = torbi_amd.decode_k_best(*args, k, route='auto')
    want = torbi_amd.decode_k_best(*args, k, route='dense')
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    # a band the LDS cannot hold at this k
    S, k = 1440, 13
    assert not bc.covered(S, k, 87, 87)
    obs, _, init = synth.problem(1, 2, S, seed=1)
    args = [torch.as_tensor(a).to(DEV) for a in (obs, np.array([2], dtype=np.int32), pitch(S, False), init)]
    with pytest.raises(RuntimeError, match='torbi_hip_k_best_band_covers'):
        torbi_amd.decode_k_best(*args, k, route='band')
    with pytest.raises(RuntimeError, match='does not cover'):
        torbi_amd.decode_k_best_banded(*args, k, 87, 87)
    assert torbi_amd.k_best_route(args[2], 1, 2, S, k, gpu=0, log_probs=True) == 'dense'
    with pytest.raises(ValueError):
        torbi_amd.decode_k_best(*args, 4, route='bogus')
    assert torbi_amd.k_best_route(None, 1, 2, S, 4, gpu=0) == 'uniform'


def test_graph_capture_with_a_caller_workspace():
    """Captured after the matrix has been looked at (`k_best_route`), replayed three times on new observations with plain
    calls in between: what a user who asks for the route first and then captures does."""
    B, T, S, k, reach, background = 9, 10, 256, 4, (5, 2), bc.TINY
    obs, trans, init = bc.model(B, T, S, 31, reach, background)
    frames = torch.tensor(ragged(B, T, 3), device=DEV)
    A, pi, x = torch.tensor(trans, device=DEV), torch.tensor(init, device=DEV), torch.tensor(obs, device=DEV)
    assert torbi_amd.k_best_route(A, B, T, S, k, gpu=0, log_probs=True) == 'band'
    assert torbi_amd.viterbi.band_over(A, A, S) == (5, 2, background)
    need = torbi_amd.decode_k_best_banded_workspace_bytes(B, T, S, k, *reach)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    torbi_amd.decode_k_best(x, frames, A, pi, k, workspace=ws)                    # warm-up outside the capture: 'auto'
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torbi_amd.decode_k_best(x, frames, A, pi, k, workspace=ws)          # 'auto' on a known band: the band route
    for seed in (32, 33, 34):
        x.copy_(torch.tensor(bc.model(B, T, S, seed, reach, background)[0], device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = torbi_amd.decode_k_best(x, frames, A, pi, k, route='dense')
        assert torch.equal(out[0], want[0]) and torch.equal(out[1].view(torch.int32), want[1].view(torch.int32))
        banded = torbi_amd.decode_k_best_banded(x, frames, A, pi, k, *reach, background)
        assert torch.equal(out[0], banded[0]) and torch.equal(out[1].view(torch.int32), banded[1].view(torch.int32))
    with pytest.raises(RuntimeError, match='workspace'):
        torbi_amd.decode_k_best_banded(x, frames, A, pi, k, *reach, background, workspace=ws[:need - 1])


def test_band_raises_without_a_matrix():
    obs, _, init = synth.problem(2, 3, 64, seed=1)
    with pytest.raises(RuntimeError, match='uniform'):
        torbi_amd.decode_k_best(torch.as_tensor(obs).to(DEV), None, None, torch.as_tensor(init).to(DEV), 2, route='band')
    with pytest.raises(RuntimeError, match='uniform'):
        torbi_amd.best_paths(torch.as_tensor(obs), 2, log_probs=True, gpu=0, route='band')
