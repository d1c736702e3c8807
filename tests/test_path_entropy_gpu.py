"""Path entropy on an MI355X (csrc/path_entropy.hpp behind torbi_hip_path_entropy / _uniform): the device routes against the
float64 host route on entropy, every prefix entry and the log-likelihood, and against the enumeration of every path
(tests/path_entropy_cases.py); -inf matrices, the non-finite rules, an item's bits inside a batch, the caller-owned
workspace, graph capture, another stream, the operand forms and the uniform route's register-row edge.

The step kernel computes a tile of STATE_TILE states x ITEM_TILE items (pe::kStateTile, pe::kItemTile; one MFMA column per
item for p and for u, so the item edge is at 32) and splits K over waves_of(S) waves in 8-wide chunks; with at least two
tiles per compute unit and four waves it stages BLOCK_K-wide blocks of its four operands through LDS (pe::kBlockK), else the
waves read global memory.  One partial sum of a_t per ROWS_PER_PARTIAL states.  Operand rows are read as float4 whatever the
states (they live padded in the workspace): 1441 states is the odd row whose last float4 lies in the padding.

The bound on H and on every prefix entry against the float64 host route is RTOL_H |ref| + ATOL_H_PER_FRAME F (prefix_t:
F = t + 1).  It was not fixed in advance: the worst error measured on the shapes of this table, softmax rows of scale 3 on a
column-normalised matrix, was 1.80 in units of 1e-6 |ref| + 1e-6 F (40 x 500 x 200, a prefix entry; ENTROPY.md has every
shape), and the bound is eleven times that.  Each test prints the figure it measured."""
import math

import numpy as np
import pytest
import torch

from torbi_amd import _lib, entropy

import operand_form_cases as ofc
import path_entropy_cases as pec
from workspace_cases import DEV, assert_guards_intact, assert_same_bits, guarded

pytestmark = pytest.mark.gpu

STATE_TILE, ITEM_TILE, BLOCK_K, ROWS_PER_PARTIAL, CHUNK, MAX_WAVES = 32, 32, 64, 32, 8, 4
ROW_REGISTERS = 2048                     # states of a uniform-route row held in registers
RTOL_H, ATOL_H_PER_FRAME = 2e-5, 2e-5
SHAPES = [(1, 1, 1), (2, 4, 1), (2, 3, 2), (15, 2, 31), (16, 3, 32), (17, 3, 33), (31, 3, 33), (32, 2, 65), (33, 64, 65),
          (1, 64, 1441), (5500, 3, 65), (600, 2, 1441), (3, 50, 200), (5, 30, 1441), (40, 500, 200)]


def waves_of(S):
    """pe::waves_of."""
    return MAX_WAVES if S >= CHUNK * MAX_WAVES else (2 if S >= 16 else 1)


def staged(B, S):
    """The step launches of a (B, ., S) call stage their operands through LDS."""
    tiles = -(-S // STATE_TILE) * -(-B // ITEM_TILE)
    return waves_of(S) == MAX_WAVES and tiles >= 2 * _lib.load().torbi_hip_compute_units(0)


def device(obs, frames, A, pi, workspace=None, prefix=True):
    out = entropy.forward_entropy(*pec.tensors(obs, frames, A, pi, device=DEV), workspace=workspace, prefix=prefix)
    torch.cuda.synchronize()
    return out


def host64(obs, frames, A, pi):
    o, f, a, p = pec.tensors(obs, frames, A, pi)
    uniform = None if A is not None else float(pec.uniform_value(np.asarray(obs).shape[2]))
    return tuple(x.numpy() for x in entropy._host(o, f, a, uniform, p))


def host_copy(out):
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def check(got, want, frames, what):
    """(entropy, log-likelihood, prefix) of the device within the bounds of the float64 `want`; prints the worst errors."""
    H, L, prefix = pec.numpy(got)
    assert all(x.dtype == torch.float32 and x.device == DEV for x in got)
    T = prefix.shape[1]
    F = pec.clamp(frames, T).astype(np.float64)
    upto = np.minimum(np.arange(1, T + 1, dtype=np.float64)[None, :], F[:, None])
    worst = (pec.close(H, want[0], RTOL_H * np.abs(want[0]) + ATOL_H_PER_FRAME * F, (what, 'entropy')),
             pec.close(prefix, want[2], RTOL_H * np.abs(want[2]) + ATOL_H_PER_FRAME * upto, (what, 'prefix')),
             pec.close(L, want[1], pec.likelihood_bound(want[1], frames, T), (what, 'log-likelihood')))
    beyond = np.arange(T)[None, :] >= F[:, None]
    assert (prefix[beyond] == 0).all(), (what, 'prefix entries t >= F are 0')
    print(f'{what}: worst error of entropy {worst[0]:.3e}, prefix {worst[1]:.3e}, log-likelihood {worst[2]:.3e}')


def test_the_shapes_cross_every_tile_edge():
    states = {S for _, _, S in SHAPES}
    assert {1, 2, 31, 32, 33, 65, 1441} <= states and {1, 15, 16, 17, 33} <= {B for B, _, _ in SHAPES}
    assert {1, 2, 3, 64} <= {T for _, T, _ in SHAPES}
    assert {STATE_TILE - 1, STATE_TILE, STATE_TILE + 1} <= states and STATE_TILE == ROWS_PER_PARTIAL
    assert {ITEM_TILE - 1, ITEM_TILE, ITEM_TILE + 1} <= {B for B, _, _ in SHAPES}
    assert any(B > ITEM_TILE and B % ITEM_TILE and S > 2 * STATE_TILE and S % STATE_TILE for B, _, S in SHAPES)
    assert {waves_of(S) for S in states} == {1, 2, 4}
    assert any(S % 4 for S in states if S > BLOCK_K)             # the last float4 of an operand row lies in the padding
    # both forms of the step launch, the staged one with a last K block that is not full and with more than one block
    assert any(staged(B, S) and S % BLOCK_K and S > BLOCK_K for B, _, S in SHAPES)
    assert any(not staged(B, S) and waves_of(S) == MAX_WAVES and B == 1 for B, _, S in SHAPES)      # split K, one item


@pytest.mark.parametrize('matrix', ['dense', None], ids=['dense', 'uniform'])
@pytest.mark.parametrize('B,T,S', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_device_against_the_float64_host_route(B, T, S, matrix):
    obs, frames, A, pi = pec.softmax_case(B, T, S, 7 * S + T, matrix=matrix)
    assert frames[0] == T and (B < 2 or frames[-1] == 1)
    got = device(obs, frames, A, pi)
    assert got[0].shape == got[1].shape == (B,) and got[2].shape == (B, T)
    check(got, host64(obs, frames, A, pi), frames, (B, T, S, matrix))
    short = device(obs, frames, A, pi, prefix=False)
    assert len(short) == 2
    assert_same_bits(host_copy(short), host_copy(got[:2]), 'without the prefix output')


@pytest.mark.parametrize('matrix', pec.KINDS, ids=[str(k) for k in pec.KINDS])
@pytest.mark.parametrize('S,T', pec.ENUMERATED, ids=[f'S{S}-T{T}' for S, T in pec.ENUMERATED])
def test_device_against_the_enumeration_of_every_path(S, T, matrix):
    obs, frames, A, pi, want = pec.enumerated_case(S, T, matrix)
    got = device(obs, frames, A, pi)
    check(got, want, frames, (S, T, matrix))
    if S == 1:
        assert (got[0] == 0).all() and (got[2] == 0).all()


@pytest.mark.parametrize('B,T,S', [(17, 3, 33), (33, 64, 65), (3, 50, 200)])
@pytest.mark.parametrize('matrix', ['left_to_right', 'permutation'])
def test_matrices_with_minus_inf_cells(matrix, B, T, S):
    obs, frames, A, pi = pec.softmax_case(B, T, S, 7 * S + T, matrix=matrix)
    assert np.isneginf(A).any()
    got = device(obs, frames, A, pi)
    assert not any(torch.isnan(x).any() for x in got)
    check(got, host64(obs, frames, A, pi), frames, (matrix, B, T, S))


def test_a_state_no_path_reaches_contributes_nothing_and_makes_no_nan():
    B, T, S = 5, 6, 70
    obs, frames, _, pi = pec.softmax_case(B, T, S, 5, matrix='dense')
    start = np.full_like(pi, -np.inf)
    start[10] = -0.5                                             # every path starts in state 10 and never goes below it
    A = pec.left_to_right(S, 3)
    got = device(obs, frames, A, start)
    assert not any(torch.isnan(x).any() for x in got) and (got[2][:, 0] == 0).all()
    check(got, host64(obs, frames, A, start), frames, 'left to right from one state')
    # a permutation matrix from one state: one path, entropy exactly 0 at every frame
    got = device(obs, frames, pec.permutation(S, 3), start)
    assert (got[0] == 0).all() and (got[2] == 0).all() and torch.isfinite(got[1]).all()


@pytest.mark.parametrize('value', [math.nan, math.inf])
@pytest.mark.parametrize('where', ['observation', 'observation_beyond', 'initial', 'matrix', 'uniform_observation',
                                   'uniform_initial'])
def test_non_finite_rule(where, value):
    B, T, S = 4, 5, 70
    uniform = where.startswith('uniform')
    obs, _, A, pi = pec.softmax_case(B, T, S, 21, matrix=None if uniform else 'dense')
    frames = np.array([5, 3, 1, 4], np.int32)
    clean = host_copy(device(obs, frames, A, pi))
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
    H, L, prefix = host_copy(device(obs, frames, A, pi))
    for b in range(B):
        f = int(frames[b])
        if b in bad:
            assert torch.isnan(H[b]) and torch.isnan(L[b]) and torch.isnan(prefix[b, :f]).all() and (prefix[b, f:] == 0).all()
        else:                                                    # the neighbours' bits do not change
            assert_same_bits((H[b:b + 1], L[b:b + 1], prefix[b]), (clean[0][b:b + 1], clean[1][b:b + 1], clean[2][b]), (where, b))


@pytest.mark.parametrize('matrix', ['dense', None], ids=['dense', 'uniform'])
def test_an_item_of_total_probability_zero(matrix):
    B, T, S = 3, 4, 70
    obs, _, A, pi = pec.softmax_case(B, T, S, 3, matrix=matrix)
    frames = np.array([4, 4, 2], np.int32)
    clean = host_copy(device(obs, frames, A, pi))
    obs = np.array(obs)
    obs[1, 2, :] = -np.inf                                       # no state can emit frame 2 of item 1
    H, L, prefix = host_copy(device(obs, frames, A, pi))
    assert L[1] == -math.inf and torch.isnan(H[1]) and torch.isnan(prefix[1]).all()
    for b in (0, 2):
        assert_same_bits((H[b:b + 1], L[b:b + 1], prefix[b]), (clean[0][b:b + 1], clean[1][b:b + 1], clean[2][b]), b)


@pytest.mark.parametrize('S,matrix', [(65, 'dense'), (20, 'dense'), (7, 'dense'), (1441, 'dense'), (68, None), (65, None)])
def test_an_item_alone_has_the_bits_it_has_inside_a_batch_of_nan(S, matrix):
    B, T = 40, 7
    obs, _, A, pi = pec.softmax_case(1, T, S, 13 * S, matrix=matrix)
    alone = host_copy(device(obs, [T], A, pi))
    for at in (0, 37):
        batch = np.full((B, T, S), np.nan, np.float32)
        batch[at] = obs[0]
        H, L, prefix = host_copy(device(batch, [T] * B, A, pi))
        assert_same_bits((H[at:at + 1], L[at:at + 1], prefix[at:at + 1]), alone, (S, matrix, at))
        others = [b for b in range(B) if b != at]
        assert torch.isnan(H[others]).all() and torch.isnan(L[others]).all() and torch.isnan(prefix[others]).all()


def test_the_staged_form_has_the_bits_of_the_direct_form():
    B, T, S = 5500, 3, 65
    obs, frames, A, pi = pec.softmax_case(B, T, S, 7 * S + T)
    assert staged(B, S) and not staged(40, S)
    whole = host_copy(device(obs, frames, A, pi))
    part = host_copy(device(obs[:40], frames[:40], A, pi))
    assert_same_bits(tuple(x[:40] for x in whole), part, 'the first 40 items of 5500, alone')


# ------------------------------------------------------------------------------------------------ the caller's workspace
WORKSPACE_CASES = {'dense-67x3x130': (67, 3, 130, 'dense'), 'dense-3x6x70': (3, 6, 70, 'dense'), 'uniform-3x6x70': (3, 6, 70, None),
                   'uniform-5x4x72': (5, 4, 72, None)}


@pytest.mark.parametrize('name', list(WORKSPACE_CASES))
def test_workspace_contract(name):
    """Exactly the queried bytes, at a 256-byte aligned base and one byte past it (the layout rounds the base up, so both are
    taken); over 0x00 and 0xFF; after a call whose inputs are NaN; a byte short raises before anything is launched."""
    B, T, S, matrix = WORKSPACE_CASES[name]
    obs, frames, A, pi = pec.softmax_case(B, T, S, 7 * S + T, matrix=matrix)
    need = entropy.path_entropy_workspace_bytes(B, T, S, uniform=matrix is None)
    fresh = host_copy(device(obs, frames, A, pi))
    check(device(obs, frames, A, pi), host64(obs, frames, A, pi), frames, name)
    for offset, fill in ((0, 0xC3), (1, 0x00), (1, 0xFF)):
        for prefix in (True, False):
            ws = guarded(need, offset=offset, fill=fill)
            got = host_copy(device(obs, frames, A, pi, workspace=ws, prefix=prefix))
            assert_same_bits(got, fresh[:len(got)], (name, offset, fill, prefix))
            assert_guards_intact(ws)
    ws = guarded(need, offset=1, fill=0xFF)
    dirty_obs, dirty_pi = np.array(obs), np.full_like(pi, np.nan)
    dirty_obs[0, min(1, T - 1), 5] = np.nan
    flagged = host_copy(device(dirty_obs, frames, A, dirty_pi, workspace=ws))
    assert torch.isnan(flagged[0]).all() and torch.isnan(flagged[1]).all()
    assert_same_bits(host_copy(device(obs, frames, A, pi, workspace=ws)), fresh, (name, 'after a call that left NaN behind'))
    assert_guards_intact(ws)
    ws = guarded(need, fill=0x5A)
    with pytest.raises(RuntimeError, match='workspace'):
        device(obs, frames, A, pi, workspace=ws[:need - 1])
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all())                              # nothing was launched
    assert_guards_intact(ws)


def test_an_empty_batch_launches_nothing():
    H, L, prefix = entropy.forward_entropy(torch.empty(0, 3, 4, device=DEV), None, None, torch.zeros(4, device=DEV), prefix=True)
    assert H.shape == L.shape == (0,) and prefix.shape == (0, 3) and H.device == DEV


# ------------------------------------------------------------------------------------------------ graphs and streams
@pytest.mark.parametrize('matrix', ['dense', None], ids=['dense', 'uniform'])
def test_graph_capture_and_two_replays_on_new_observations(matrix):
    B, T, S = 5, 7, 65
    first, frames, A, pi = pec.softmax_case(B, T, S, 31, matrix=matrix)
    obs, f, A_, pi_ = pec.tensors(first, frames, A, pi, device=DEV)
    ws = torch.empty(entropy.path_entropy_workspace_bytes(B, T, S, uniform=matrix is None), dtype=torch.uint8, device=DEV)
    entropy.forward_entropy(obs, f, A_, pi_, workspace=ws, prefix=True)        # (loads the kernels outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = entropy.forward_entropy(obs, f, A_, pi_, workspace=ws, prefix=True)
    for seed in (32, 33):
        again = pec.softmax_case(B, T, S, seed, matrix=matrix)[0]
        obs.copy_(torch.from_numpy(again))
        graph.replay()
        torch.cuda.synchronize()
        want = entropy.forward_entropy(obs.clone(), f, A_, pi_, prefix=True)
        assert_same_bits(host_copy(out), host_copy(want), 'a replayed graph against a fresh call')
        check(out, host64(again, frames, A, pi), frames, ('replay', seed))


def test_a_call_on_another_stream():
    B, T, S = 5, 7, 65
    obs, frames, A, pi = pec.softmax_case(B, T, S, 7 * S + T)
    ops = pec.tensors(obs, frames, A, pi, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = entropy.forward_entropy(*ops, prefix=True)
    stream.synchronize()
    check(out, host64(obs, frames, A, pi), frames, 'another stream')


# ------------------------------------------------------------------------------------------------ the front
def test_path_entropy_takes_probabilities_and_writes_nothing():
    B, T, S = 9, 6, 70
    g = torch.Generator().manual_seed(3)
    obs = torch.softmax(3 * torch.randn(B, T, S, generator=g), 2)
    A = torch.softmax(torch.randn(S, S, generator=g), 0)
    pi = torch.softmax(torch.randn(S, generator=g), 0)
    frames = torch.from_numpy(pec.ragged(B, T, 3))
    before = obs.clone()
    for matrix in (A, None):
        got = entropy.path_entropy(obs, frames, matrix, pi, gpu=0, prefix=True)
        want = entropy.path_entropy(obs, frames, matrix, pi, gpu=None, prefix=True)
        assert torch.equal(obs, before) and len(entropy.path_entropy(obs, frames, matrix, pi, gpu=0)) == 2
        check(got, tuple(x.double().numpy() for x in (want[0], want[1], want[2])), frames.numpy(), 'path_entropy')


# ------------------------------------------------------------------------------------------------ the uniform route's rows
@pytest.mark.parametrize('S', [1, 7, ROW_REGISTERS, ROW_REGISTERS + 1])
def test_uniform_route_around_the_register_row(S):
    B, T = 3, 4
    obs, frames, _, pi = pec.softmax_case(B, T, S, 11 * S + T, matrix=None)
    got = device(obs, frames, None, pi)
    check(got, host64(obs, frames, None, pi), frames, ('uniform', S))
    if S == 1:
        assert (got[0] == 0).all() and (got[2] == 0).all()
    # an observation whose rows are not 16-byte aligned takes the other form of the row kernel: the same bits
    o, f, p = pec.tensors(obs, frames, pi, device=DEV)
    shifted = torch.empty(o.numel() + 7, device=DEV)[1:1 + o.numel()].view(o.shape).copy_(o)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert_same_bits(host_copy(entropy.forward_entropy(shifted, f, None, p, prefix=True)), host_copy(got), ('unaligned', S))


# ------------------------------------------------------------------------------------------------ operand forms
FORM_CASES = pec.form_cases(DEV)


@pytest.mark.parametrize('name,operand,form_name', FORM_CASES, ids=['-'.join(c) for c in FORM_CASES])
def test_a_form_equals_its_plain_copy_and_nothing_is_written(name, operand, form_name):
    ofc.check_forms(pec.ENTRY[name], DEV, 0, {operand: form_name})


@pytest.mark.parametrize('name', list(pec.ENTRY))
def test_every_operand_in_another_form_at_once(name):
    entry = pec.ENTRY[name]
    ofc.check_forms(entry, DEV, 0, {operand: ofc.TOGETHER[operand] for operand in entry.operands})
