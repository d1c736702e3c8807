"""The band route of max-marginals on an MI355X (csrc/max_marginals_band.hpp behind torbi_hip_max_marginals_band): the device
against the full-row numpy loop of the contract (`max_marginal_cases.loop` on the whole matrix), by value with equal NaN
positions and no tolerance; both terms of the rule, unreachable states, exact grid inputs, the non-finite rule and the
promise, the routes of `max_marginals`, the caller-owned workspace, graph capture, another stream and the operand forms.

mmb_kernel<G> runs 1024 threads per workgroup (mbc.THREADS): a thread owns states tid, tid + 1024, ..., so 64 states are one
wave, 68 a partial second wave, 1028 give four threads a second state and 3072 every thread three.  A workgroup owns G items,
G from 4 halved while the launch has fewer than 256 workgroups (mbc.items_per_workgroup): batches up to 510 run G = 1, 1020
runs G = 2 and 1021 runs G = 4 with a partial last tile."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import inputs, margins

import max_marginal_band_cases as mbc
import max_marginal_cases as mmc
import operand_form_cases as ofc
import stream_band_cases as sbc
from workspace_cases import DEV, assert_guards_intact, assert_same_bits, guarded

pytestmark = pytest.mark.gpu

# (B, T, S, reach_left, reach_right): every reach at the floor; a partial wave; reach 31/31; a thread with two states; the widest
# window at the most states; one frame; every G with a partial tile
SHAPES = ([(5, 6, S, left, right) for S, left, right in mbc.REACH_CASES]
          + [(9, 6, 68, 3, 2), (5, 5, 132, 31, 31), (1, 6, 132, 0, 3), (5, 4, 1028, 3, 2), (1, 3, 1028, 2, 5), (1, 3, 3072, 254, 254),
             (1, 3, 3072, 0, 508), (5, 1, 64, 3, 2), (1, 1, 68, 2, 2), (1020, 3, 64, 3, 2), (1021, 3, 64, 2, 5)])


def device(obs, frames, A, pi, left, right, background, workspace=None):
    out = margins.forward_backward_max_banded(*mmc.tensors(obs, frames, A, pi, device=DEV), left, right, float(background),
                                              workspace=workspace)
    torch.cuda.synchronize()
    return out


def host_copy(out):
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def test_the_shapes_reach_every_instance_and_edge():
    assert {mbc.items_per_workgroup(B, S, left, right) for B, _, S, left, right in SHAPES} == {1, 2, 4}
    assert any(B % 4 and mbc.items_per_workgroup(B, S, left, right) == 4 for B, _, S, left, right in SHAPES)
    assert {B for B, *_ in SHAPES} >= {1, 5, 9}
    assert any(S % 64 for *_, S, _, _ in SHAPES) and any(mbc.THREADS < S < 2 * mbc.THREADS for *_, S, _, _ in SHAPES)
    assert any(S == 3072 and left + right + 4 == 512 for *_, S, left, right in SHAPES) and any(T == 1 for _, T, *_ in SHAPES)


@pytest.mark.parametrize('background', list(mbc.BACKGROUNDS))
@pytest.mark.parametrize('B,T,S,left,right', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_device_equals_the_full_row_loop(B, T, S, left, right, background):
    obs, frames, A, pi, want = mbc.case(B, T, S, left, right, background, seed=S + left)
    assert frames[0] == T and (B < 2 or frames[-1] == 1)
    got = device(obs, frames, A, pi, left, right, mbc.BACKGROUNDS[background])
    assert got[0].shape == (B, T, S) and got[1].shape == (B,) and got[0].device == DEV
    mmc.same(got, want, (B, T, S, left, right, background))


def test_both_terms_decide_and_the_device_equals_the_loop():
    """The inputs on which the out-of-band term strictly decides at least a quarter of the cells of each pass, and the
    in-band term at least a quarter: a wrong prefix or suffix maximum changes values here."""
    B, T, S, left, right, background = mbc.BOTH_TERMS
    obs, frames, A, pi, want = mbc.case(*mbc.BOTH_TERMS)
    decided = mbc.restate(obs, frames, A, pi, left, right, mbc.BACKGROUNDS[background])[2]
    for which, (out, inside) in mbc.decided_shares(decided).items():
        assert out >= .25 and inside >= .25, (which, out, inside)
    mmc.same(device(obs, frames, A, pi, left, right, mbc.BACKGROUNDS[background]), want)
    # the same background where a thread owns two states and the runs of the scans are two states long
    obs, frames, A, pi, want = mbc.case(3, 4, 1028, 3, 2, 'minus_3', seed=9)
    mmc.same(device(obs, frames, A, pi, 3, 2, -3.), want, 1028)


@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny'])
def test_unreachable_states_are_minus_inf(background):
    B, T, S = 5, 6, 72
    bg = mbc.BACKGROUNDS[background]
    obs, frames, _, pi, _ = mmc.softmax_case(B, T, S, 5)
    A = sbc.band_matrix(S, 2, 1, bg, seed=3)
    pi = np.full_like(pi, -np.inf)
    pi[10] = -0.5                                                # every path starts in state 10
    want = mmc.loop(obs, frames, A, pi)
    got = device(obs, frames, A, pi, 2, 1, bg)
    mmc.same(got, want, background)
    m = got[0].cpu().numpy()
    assert not np.isnan(m).any() and np.isfinite(got[1].cpu().numpy()).all()
    unreachable = np.isneginf(m[0, :, :])                        # item 0 has every frame
    if np.isneginf(bg):
        # prev i reaches next j for j - 2 <= i <= j + 1: from state 10 a path is within [10 - t, 10 + 2 t] at frame t
        for t in range(T):
            assert not unreachable[t, 10 - t:10 + 2 * t + 1].any() and unreachable[t, :10 - t].all() and unreachable[t, 11 + 2 * t:].all()
    else:
        assert not unreachable[1:].any() and unreachable[0].sum() == S - 1


@pytest.mark.parametrize('left,right', [(3, 2), (31, 31)])
def test_grid_inputs_are_path_consistent_and_the_score_is_best_paths(left, right):
    """Every sum is exact on the -0.25 grid, the background (a grid value inside the in-band range) included: max_j m_t[j] ==
    score at every frame, and the score is `best_paths(k=1, route='dense')`'s bit for bit."""
    B, T, S = 5, 6, 64
    bg = float(sbc.tie_background(left, right))
    obs, frames, A, pi, want = mbc.case(B, T, S, left, right, bg, seed=13, grid=4)
    # (the grid's zeros are -0; `best_paths` below reads them as +0 behind its epsilon round trip, and the sign of a zero is
    # the one thing the values leave open, so both get +0)
    obs, A, pi = obs + np.float32(0), A + np.float32(0), pi + np.float32(0)
    got = device(obs, frames, A, pi, left, right, bg)
    mmc.same(got, want, 'grid')
    mmc.check_path_consistency(got, frames, 'grid')
    o, f, a, p = mmc.tensors(obs, frames, A, pi)
    # (the epsilon round trip of `log_probs=True` returns grid values unchanged: sbc.grid_scores)
    _, best = torbi_amd.best_paths(o, 1, f, a, p, log_probs=True, gpu=0, route='dense')
    best = best[:, 0].contiguous().view(torch.int32)
    assert torch.equal(got[1].view(torch.int32), best)
    if bg < -0.75:                                               # the background is no in-band value: the band is found as stated
        m, score = margins.max_marginals(o, f, a, p, log_probs=True, gpu=0, route='band')
        mmc.check_path_consistency((m, score), frames, 'grid through max_marginals')
        assert torch.equal(score.view(torch.int32), best)


@pytest.mark.parametrize('background', ['minus_inf', 'minus_3'])
@pytest.mark.parametrize('value', [math.nan, math.inf])
@pytest.mark.parametrize('where', ['observation', 'observation_beyond', 'initial', 'matrix'])
def test_non_finite_rule(where, value, background):
    B, T, S, left, right = 4, 5, 68, 3, 2
    bg = mbc.BACKGROUNDS[background]
    obs, _, A, pi, _ = mbc.case(B, T, S, left, right, background, seed=21)
    frames = np.array([5, 3, 1, 4], np.int32)
    clean = device(obs, frames, A, pi, left, right, bg)
    mmc.same(clean, mmc.loop(obs, frames, A, pi), 'clean')
    obs, pi, A = np.array(obs), np.array(pi), np.array(A)
    if where == 'observation':
        obs[1, 2, 67] = value                                    # item 1, inside its 3 frames
        bad = [1]
    elif where == 'observation_beyond':
        obs[1, 3, 4] = value                                     # item 1, behind its frames: nobody reads it
        bad = []
    elif where == 'initial':
        pi[2] = value
        bad = [0, 1, 2, 3]
    else:
        A[3, 1] = value                                          # inside the band
        bad = [0, 1, 3]                                          # item 2 has one frame and reads no matrix
    got = device(obs, frames, A, pi, left, right, bg)
    mmc.same(got, mmc.loop(obs, frames, A, pi), where)
    m, score = (x.cpu() for x in got)
    for b in range(B):
        f = int(frames[b])
        if b in bad:
            assert torch.isnan(m[b, :f]).all() and torch.isnan(score[b]) and (m[b, f:] == -math.inf).all()
        else:                                                    # the neighbours' bits do not change
            assert_same_bits((m[b], score[b:b + 1]), (clean[0][b].cpu(), clean[1][b:b + 1].cpu()), (where, b))


@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny'])
def test_a_broken_promise_gives_every_item_nan(background):
    """One stray entry outside the band: every item, the one of a single frame included, has NaN rows and a NaN score."""
    B, T, S, left, right = 4, 5, 68, 3, 2
    bg = mbc.BACKGROUNDS[background]
    obs, _, A, pi, _ = mbc.case(B, T, S, left, right, background, seed=21)
    frames = np.array([5, 3, 1, 4], np.int32)
    stray = np.array(A)
    stray[40, 3] = np.float32(-1.)
    m, score = (x.cpu() for x in device(obs, frames, stray, pi, left, right, bg))
    for b in range(B):
        f = int(frames[b])
        assert torch.isnan(m[b, :f]).all() and torch.isnan(score[b]) and (m[b, f:] == -math.inf).all(), b
    want = mbc.restate(obs, frames, stray, pi, left, right, bg)
    mmc.same((m, score), want[:2], 'the restatement of the promise')
    # a stray value that differs in the sign bit alone
    if background == 'log_tiny':
        stray = np.array(A)
        stray[40, 3] = -stray[40, 3]
        assert torch.isnan(device(obs, frames, stray, pi, left, right, bg)[1]).all()


# ------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny', 'minus_3'])
def test_routes_of_max_marginals_agree(background):
    B, T, S, left, right = 5, 6, 68, 3, 2
    obs, frames, A, pi, _ = mbc.case(B, T, S, left, right, background, seed=4)
    o, f, a, p = mmc.tensors(obs, frames, A, pi)
    dense = host_copy(margins.max_marginals(o, f, a, p, log_probs=True, gpu=0, route='dense'))
    assert not torch.isnan(dense[1]).any()
    for route in ('band', 'auto'):
        got = host_copy(margins.max_marginals(o, f, a, p, log_probs=True, gpu=0, route=route))
        mmc.same(got, [x.numpy() for x in dense], route)
    # `max_marginals_route` answers what 'auto' takes: the band the look finds, where it pays.  The look (`viterbi.band_over`)
    # answers the stated band for -inf outside it; for a finite value it does so only where every other entry lies above that
    # value, and these in-band scores reach below -3: there it answers the whole row, S - 1 / S - 1 -- a band that is true,
    # that 'band' above ran and that no class of `_AUTO_BAND` holds.
    trans = inputs.device_matrix(a, True, DEV)
    band, why = margins._band_plan(trans, trans, 512, 500, S, 0)
    assert band is not None and band[0] >= left and band[1] >= right, why
    assert margins.max_marginals_route(a, 512, 500, S, gpu=0, log_probs=True) == (
        'band' if margins._band_pays(512, S, band[0], band[1]) else 'dense')
    if background != 'minus_3':
        assert band == (left, right, float(mbc.BACKGROUNDS[background]))
        assert margins.max_marginals_route(a, B, T, S, gpu=0, log_probs=True) == 'band'
    else:
        assert band == (S - 1, S - 1, -3.) and margins.max_marginals_route(a, B, T, S, gpu=0, log_probs=True) == 'dense'


def test_band_raises_with_the_planner_s_reason_where_there_is_no_covered_band():
    B, T, S = 3, 4, 70                                           # 70 % 4 != 0: viterbi.band_over cannot answer
    obs, frames, _, pi, _ = mmc.softmax_case(B, T, S, 5)
    A = sbc.band_matrix(S, 2, 1, -np.inf, seed=3)
    o, f, a, p = mmc.tensors(obs, frames, A, pi)
    with pytest.raises(RuntimeError) as raised:
        margins.max_marginals(o, f, a, p, log_probs=True, gpu=0, route='band')
    assert str(raised.value).startswith("max_marginals(route='band'): the matrix does not hold one value outside a band")
    dense = host_copy(margins.max_marginals(o, f, a, p, log_probs=True, gpu=0, route='dense'))
    mmc.same(host_copy(margins.max_marginals(o, f, a, p, log_probs=True, gpu=0, route='auto')), [x.numpy() for x in dense])
    with pytest.raises(RuntimeError, match='forward_backward_max_banded does not cover'):
        margins.forward_backward_max_banded(o.to(DEV), f, a, p, 2, 1)


# ------------------------------------------------------------------------------------------------ the caller's workspace
WORKSPACE_CASES = {'minus_inf-9x6x68': (9, 6, 68, 3, 2, 'minus_inf'), 'minus_3-5x4x132': (5, 4, 132, 31, 31, 'minus_3'),
                   'log_tiny-3x5x1028': (3, 5, 1028, 2, 5, 'log_tiny')}


@pytest.mark.parametrize('name', list(WORKSPACE_CASES))
def test_workspace_contract(name):
    """Exactly the queried bytes, at a 256-byte aligned base and one byte past it; over 0x00, 0xFF and what earlier calls left;
    after a call whose inputs raise every alarm and after a broken promise; a byte short raises before anything is launched."""
    B, T, S, left, right, background = WORKSPACE_CASES[name]
    bg = mbc.BACKGROUNDS[background]
    obs, frames, A, pi, want = mbc.case(B, T, S, left, right, background, seed=7 * S + T)
    need = margins.max_marginals_banded_workspace_bytes(B, T, S, left, right)
    fresh = host_copy(device(obs, frames, A, pi, left, right, bg))
    mmc.same(fresh, want, name)
    for offset, fill in ((0, 0xC3), (1, 0x00), (1, 0xFF)):
        ws = guarded(need, offset=offset, fill=fill)
        assert_same_bits(host_copy(device(obs, frames, A, pi, left, right, bg, workspace=ws)), fresh, (name, offset, fill))
        assert_guards_intact(ws)
    ws = guarded(need, offset=1, fill=0xFF)
    dirty_obs, dirty_pi = np.array(obs), np.full_like(pi, np.nan)
    dirty_obs[0, min(1, T - 1), 5] = np.nan
    dirty_A = np.array(A)
    dirty_A[4, 4] = np.inf
    flagged = host_copy(device(dirty_obs, frames, dirty_A, dirty_pi, left, right, bg, workspace=ws))
    assert torch.isnan(flagged[1]).all()
    flagged = host_copy(device(obs, frames, dirty_A, pi, left, right, bg, workspace=ws))
    assert torch.isnan(flagged[1][0]) and not torch.isnan(flagged[1][-1])            # (the last item has one frame)
    assert_same_bits(host_copy(device(obs, frames, A, pi, left, right, bg, workspace=ws)), fresh, (name, 'after calls that raise every alarm'))
    stray = np.array(A)
    stray[S - 1, 0] = np.float32(-2.)
    assert torch.isnan(host_copy(device(obs, frames, stray, pi, left, right, bg, workspace=ws))[1]).all()
    assert_same_bits(host_copy(device(obs, frames, A, pi, left, right, bg, workspace=ws)), fresh, (name, 'after a broken promise'))
    assert_guards_intact(ws)
    ws = guarded(need, fill=0x5A)
    with pytest.raises(RuntimeError, match='workspace'):
        device(obs, frames, A, pi, left, right, bg, workspace=ws[:need - 1])
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all())                              # nothing was launched
    assert_guards_intact(ws)


def test_an_empty_batch_launches_nothing():
    A = torch.from_numpy(sbc.band_matrix(64, 2, 2, -np.inf)).to(DEV)
    m, score = margins.forward_backward_max_banded(torch.empty(0, 3, 64, device=DEV), None, A, torch.zeros(64, device=DEV), 2, 2)
    assert m.shape == (0, 3, 64) and score.shape == (0,) and m.device == DEV


# ------------------------------------------------------------------------------------------------ graphs and streams
@pytest.mark.parametrize('background', ['minus_inf', 'minus_3'])
def test_graph_capture_and_replay_on_a_new_observation(background):
    B, T, S, left, right = 5, 7, 68, 3, 2
    bg = float(mbc.BACKGROUNDS[background])
    first, frames, A, pi, _ = mbc.case(B, T, S, left, right, background, seed=31)
    second = mbc.case(B, T, S, left, right, background, seed=32)[0]
    obs, f, A, pi = mmc.tensors(first, frames, A, pi, device=DEV)
    ws = torch.empty(margins.max_marginals_banded_workspace_bytes(B, T, S, left, right), dtype=torch.uint8, device=DEV)
    margins.forward_backward_max_banded(obs, f, A, pi, left, right, bg, workspace=ws)        # (loads the kernels outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = margins.forward_backward_max_banded(obs, f, A, pi, left, right, bg, workspace=ws)
    obs.copy_(torch.from_numpy(second))
    graph.replay()
    torch.cuda.synchronize()
    want = margins.forward_backward_max_banded(obs.clone(), f, A, pi, left, right, bg)
    assert_same_bits(host_copy(out), host_copy(want), 'a replayed graph against a fresh call')
    mmc.same(out, mmc.loop(second, frames, A.cpu().numpy(), pi.cpu().numpy()))


def test_a_call_on_another_stream():
    B, T, S, left, right = 5, 7, 68, 3, 2
    obs, frames, A, pi, want = mbc.case(B, T, S, left, right, 'minus_3', seed=31)
    ops = mmc.tensors(obs, frames, A, pi, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = margins.forward_backward_max_banded(*ops, left, right, -3.)
    stream.synchronize()
    mmc.same(out, want)


# ------------------------------------------------------------------------------------------------ operand forms
FORM_CASES = mbc.form_cases(DEV)


@pytest.mark.parametrize('name,operand,form_name', FORM_CASES, ids=['-'.join(c) for c in FORM_CASES])
def test_a_form_equals_its_plain_copy_and_nothing_is_written(name, operand, form_name):
    ofc.check_forms(mbc.ENTRY[name], DEV, 0, {operand: form_name})


@pytest.mark.parametrize('name', list(mbc.ENTRY))
def test_every_operand_in_another_form_at_once(name):
    entry = mbc.ENTRY[name]
    ofc.check_forms(entry, DEV, 0, {operand: ofc.TOGETHER[operand] for operand in entry.operands})
