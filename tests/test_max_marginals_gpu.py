"""Max-marginals on an MI355X (csrc/max_marginals.hpp behind torbi_hip_max_marginals / _uniform): the device routes against the
numpy loop of the contract and against brute-force enumeration (tests/max_marginal_cases.py), by value with equal NaN
positions; -inf matrices, the uniform collapse, `best_paths`' score, the non-finite rule, the caller-owned workspace, graph
capture, another stream and the operand forms.

The step kernel computes a tile of ITEM_TILE items x ROW_TILE rows and stages the contraction axis in chunks of CHUNK
(mm::kItemTile, mm::kRowTile, mm::kChunk).  Of the shapes below 67 x 3 x 130 exceeds one item tile (64 + 3), one row tile
(2 x 64 + 2) and two chunks (2 x 64 + 2) by a non-multiple; 17 x 4 x 64 is exactly one row tile and one chunk.  A
workgroup splits every chunk among 4, 2 or 1 groups of four waves (mm::step_groups: the fewest that bring the launch's
tiles to FULL_WAVES waves, a function of the shape alone); every shape of the table runs 4 groups, 8192 x 3 x 65 (256
tiles) runs 2 and 16384 x 3 x 65 (512 tiles) runs 1."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import margins

import max_marginal_cases as mmc
import operand_form_cases as ofc
import stream_band_cases as sbc
from workspace_cases import DEV, assert_guards_intact, assert_same_bits, guarded

pytestmark = pytest.mark.gpu

ITEM_TILE, ROW_TILE, CHUNK, FULL_WAVES = 64, 64, 64, 2048
SHAPES = [(1, 1, 1), (1, 5, 1), (2, 1, 7), (3, 6, 3), (5, 7, 65), (17, 4, 64), (67, 3, 130), (3, 5, 300), (8192, 3, 65),
          (16384, 3, 65)]


def groups(B, S):
    """mm::step_groups for a (B, ., S) call."""
    tiles = -(-B // ITEM_TILE) * -(-S // ROW_TILE)
    return next((g for g in (1, 2) if tiles * 4 * g >= FULL_WAVES), 4)


def device(obs, frames, A, pi, workspace=None):
    out = margins.forward_backward_max(*mmc.tensors(obs, frames, A, pi, device=DEV), workspace=workspace)
    torch.cuda.synchronize()
    return out


def host_copy(out):
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def test_the_shapes_cross_every_tile_edge():
    assert any(B > ITEM_TILE and B % ITEM_TILE and S > ROW_TILE and S % ROW_TILE and S > 2 * CHUNK and S % CHUNK
               for B, _, S in SHAPES)
    assert any(S == ROW_TILE == CHUNK for _, _, S in SHAPES) and any(S == 1 for _, _, S in SHAPES)
    assert {groups(B, S) for B, _, S in SHAPES} == {1, 2, 4}


@pytest.mark.parametrize('B,T,S', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_device_equals_the_numpy_loop(B, T, S):
    obs, frames, A, pi, want = mmc.softmax_case(B, T, S, 7 * S + T)
    assert frames[0] == T and (B < 2 or frames[-1] == 1)
    got = device(obs, frames, A, pi)
    assert got[0].shape == (B, T, S) and got[1].shape == (B,) and got[0].device == DEV
    mmc.same(got, want, (B, T, S))


@pytest.mark.parametrize('S,T,holes', mmc.DYADIC, ids=[f'S{S}-T{T}-holes{holes}' for S, T, holes in mmc.DYADIC])
def test_device_equals_the_enumeration_of_every_path(S, T, holes):
    obs, frames, A, pi, want = mmc.dyadic_case(mmc.DYADIC_ITEMS, T, S, 100 * S + T, holes)
    got = device(obs, frames, A, pi)
    mmc.same(got, want, (S, T, holes))
    mmc.check_path_consistency(got, frames, (S, T, holes))


@pytest.mark.parametrize('background', [sbc.BACKGROUNDS['minus_inf'], sbc.TINY], ids=['minus_inf', 'log_tiny'])
def test_band_matrix_through_the_dense_route(background):
    B, T, S = 5, 6, 70
    obs, frames, _, pi, _ = mmc.softmax_case(B, T, S, 5)
    A = sbc.band_matrix(S, 2, 1, background, seed=3)
    pi = np.full_like(pi, -np.inf)
    pi[10] = -0.5                                                # every path starts in state 10
    want = mmc.loop(obs, frames, A, pi)
    got = device(obs, frames, A, pi)
    mmc.same(got, want, background)
    m = got[0].cpu().numpy()
    assert not np.isnan(m).any() and np.isfinite(got[1].cpu().numpy()).all()
    unreachable = np.isneginf(m[0, :, :])                        # item 0 has every frame
    if np.isneginf(background):
        # prev i reaches next j for j - 2 <= i <= j + 1: from state 10 a path is within [10 - t, 10 + 2 t] at frame t
        for t in range(T):
            assert not unreachable[t, 10 - t:10 + 2 * t + 1].any() and unreachable[t, :10 - t].all() and unreachable[t, 11 + 2 * t:].all()
    else:
        assert not unreachable[1:].any() and unreachable[0].sum() == S - 1


@pytest.mark.parametrize('B,T,S', [(1, 1, 1), (2, 5, 1), (3, 6, 3), (5, 7, 65), (67, 3, 132), (3, 5, 300)])
def test_uniform_route_equals_the_dense_route_on_the_filled_matrix(B, T, S):
    obs, frames, _, pi, want = mmc.softmax_case(B, T, S, 11 * S + T, matrix=False)
    filled = np.full((S, S), mmc.uniform_value(S), np.float32)
    got = device(obs, frames, None, pi)
    mmc.same(got, want, 'uniform against the loop')
    mmc.same(got, [x.cpu().numpy() for x in device(obs, frames, filled, pi)], 'uniform against dense')


@pytest.mark.parametrize('matrix', [True, False])
def test_score_is_best_paths_score_bit_for_bit(matrix):
    B, T, S = 9, 6, 70
    g = torch.Generator().manual_seed(3)
    obs = torch.softmax(3 * torch.randn(B, T, S, generator=g), 2)
    A = torch.softmax(torch.randn(S, S, generator=g), 0) if matrix else None
    pi = torch.softmax(torch.randn(S, generator=g), 0)
    frames = torch.from_numpy(mmc.ragged(B, T, 3))
    before = obs.clone()
    m, score = margins.max_marginals(obs, frames, A, pi, gpu=0)
    _, want = torbi_amd.best_paths(obs, 1, frames, A, pi, gpu=0, route='dense')
    assert score.device == DEV and torch.equal(score.view(torch.int32), want[:, 0].contiguous().view(torch.int32))
    last = m[torch.arange(B, device=DEV), frames.to(DEV).long() - 1]
    assert torch.equal(last.amax(1), score)                      # m_{F-1} is alpha_{F-1} in value
    assert m.shape == (B, T, S) and torch.equal(obs, before)


@pytest.mark.parametrize('value', [math.nan, math.inf])
@pytest.mark.parametrize('where', ['observation', 'observation_beyond', 'initial', 'matrix', 'uniform_observation',
                                   'uniform_initial'])
def test_non_finite_rule(where, value):
    B, T, S = 4, 5, 70
    uniform = where.startswith('uniform')
    obs, _, A, pi, _ = mmc.softmax_case(B, T, S, 21, matrix=not uniform)
    frames = np.array([5, 3, 1, 4], np.int32)
    clean = device(obs, frames, A, pi)
    obs, pi = np.array(obs), np.array(pi)
    A = None if uniform else np.array(A)
    if where.endswith('observation'):
        obs[1, 2, 67] = value                                    # item 1, inside its 3 frames
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
    got = device(obs, frames, A, pi)
    mmc.same(got, mmc.loop(obs, frames, A, pi), where)
    m, score = (x.cpu() for x in got)
    for b in range(B):
        f = int(frames[b])
        if b in bad:
            assert torch.isnan(m[b, :f]).all() and torch.isnan(score[b]) and (m[b, f:] == -math.inf).all()
        else:                                                    # the neighbours' values do not change
            assert_same_bits((m[b], score[b:b + 1]), (clean[0][b].cpu(), clean[1][b:b + 1].cpu()), (where, b))


# ------------------------------------------------------------------------------------------------ the caller's workspace
WORKSPACE_CASES = {'dense-67x3x130': (67, 3, 130, True), 'dense-3x6x70': (3, 6, 70, True), 'uniform-3x6x70': (3, 6, 70, False),
                   'uniform-5x4x72': (5, 4, 72, False)}


@pytest.mark.parametrize('name', list(WORKSPACE_CASES))
def test_workspace_contract(name):
    """Exactly the queried bytes, at a 256-byte aligned base and one byte past it (the layout rounds the base up, so both are
    taken); over 0x00 and 0xFF; after a call whose inputs raise every alarm; a byte short raises before anything is launched."""
    B, T, S, matrix = WORKSPACE_CASES[name]
    obs, frames, A, pi, want = mmc.softmax_case(B, T, S, 7 * S + T, matrix=matrix)
    need = margins.max_marginals_workspace_bytes(B, T, S, uniform=not matrix)
    fresh = host_copy(device(obs, frames, A, pi))
    mmc.same(fresh, want, name)
    for offset, fill in ((0, 0xC3), (1, 0x00), (1, 0xFF)):
        ws = guarded(need, offset=offset, fill=fill)
        assert_same_bits(host_copy(device(obs, frames, A, pi, workspace=ws)), fresh, (name, offset, fill))
        assert_guards_intact(ws)
    ws = guarded(need, offset=1, fill=0xFF)
    dirty_obs, dirty_pi = np.array(obs), np.full_like(pi, np.nan)
    dirty_obs[0, min(1, T - 1), 5] = np.nan
    flagged = host_copy(device(dirty_obs, frames, A, dirty_pi, workspace=ws))
    assert torch.isnan(flagged[1]).all()
    if matrix:
        dirty_A = np.array(A)
        dirty_A[4, 4] = np.inf
        flagged = host_copy(device(obs, frames, dirty_A, pi, workspace=ws))
        assert torch.isnan(flagged[1][0]) and not torch.isnan(flagged[1][-1])        # (the last item has one frame)
    assert_same_bits(host_copy(device(obs, frames, A, pi, workspace=ws)), fresh, (name, 'after calls that raise every alarm'))
    assert_guards_intact(ws)
    ws = guarded(need, fill=0x5A)
    with pytest.raises(RuntimeError, match='workspace'):
        device(obs, frames, A, pi, workspace=ws[:need - 1])
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all())                              # nothing was launched
    assert_guards_intact(ws)


def test_an_empty_batch_launches_nothing():
    m, score = margins.forward_backward_max(torch.empty(0, 3, 4, device=DEV), None, None, torch.zeros(4, device=DEV))
    assert m.shape == (0, 3, 4) and score.shape == (0,) and m.device == DEV


# ------------------------------------------------------------------------------------------------ graphs and streams
@pytest.mark.parametrize('matrix', [True, False])
def test_graph_capture_and_replay_on_a_new_observation(matrix):
    B, T, S = 5, 7, 65
    first, frames, A, pi, _ = mmc.softmax_case(B, T, S, 31, matrix=matrix)
    second = mmc.softmax_case(B, T, S, 32, matrix=matrix)[0]
    obs, f, A, pi = mmc.tensors(first, frames, A, pi, device=DEV)
    ws = torch.empty(margins.max_marginals_workspace_bytes(B, T, S, uniform=not matrix), dtype=torch.uint8, device=DEV)
    margins.forward_backward_max(obs, f, A, pi, workspace=ws)        # (loads the kernels outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = margins.forward_backward_max(obs, f, A, pi, workspace=ws)
    obs.copy_(torch.from_numpy(second))
    graph.replay()
    torch.cuda.synchronize()
    want = margins.forward_backward_max(obs.clone(), f, A, pi)
    assert_same_bits(host_copy(out), host_copy(want), 'a replayed graph against a fresh call')
    mmc.same(out, mmc.loop(second, frames, None if A is None else A.cpu().numpy(), pi.cpu().numpy()))


def test_a_call_on_another_stream():
    B, T, S = 5, 7, 65
    obs, frames, A, pi, want = mmc.softmax_case(B, T, S, 7 * S + T)
    ops = mmc.tensors(obs, frames, A, pi, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = margins.forward_backward_max(*ops)
    stream.synchronize()
    mmc.same(out, want)


# ------------------------------------------------------------------------------------------------ operand forms
FORM_CASES = mmc.form_cases(DEV)


@pytest.mark.parametrize('name,operand,form_name', FORM_CASES, ids=['-'.join(c) for c in FORM_CASES])
def test_a_form_equals_its_plain_copy_and_nothing_is_written(name, operand, form_name):
    ofc.check_forms(mmc.ENTRY[name], DEV, 0, {operand: form_name})


@pytest.mark.parametrize('name', list(mmc.ENTRY))
def test_every_operand_in_another_form_at_once(name):
    entry = mmc.ENTRY[name]
    ofc.check_forms(entry, DEV, 0, {operand: ofc.TOGETHER[operand] for operand in entry.operands})
