"""The band route of path entropy on an MI355X (csrc/path_entropy_band.hpp behind torbi_hip_path_entropy_band): the device
against the float64 host route on the FULL matrix (`entropy._host`) on entropy, every prefix entry and the log-likelihood;
agreement with the dense device route; an item's bits inside a batch; the promise; the non-finite rules; -inf cells inside the
band; the caller-owned workspace; graph capture; another stream; the routes of `path_entropy`; the operand forms.

pe_band_kernel<G> runs 1024 threads per workgroup (pbc.THREADS): a thread owns states tid, tid + 1024, ..., so 64 states are
one wave, 65 a second wave of one lane, 1025 give one thread a second state and 1440 give 416 threads one.  A workgroup owns G
items, G from 4 (pbc.MAX_GROUP) halved while the pairs of G items do not fit 159 KB of LDS, then while the launch has fewer
workgroups than the device has compute units (pbc.items_per_workgroup): on 256 compute units batches up to 510 run G = 1,
up to 1020 G = 2, and 1023, 1024 and 1025 run G = 4 with a last tile of G - 1, G and 1 items.

The bound on H and on every prefix entry against float64 is RTOL_H |ref| + ATOL_H_PER_FRAME F (prefix_t: F = t + 1).  It
was not fixed in advance.  In units of 1e-6 |ref| + 1e-6 F the worst error measured on the shapes of this table with all
three backgrounds was 3.72 (MEASURED_WORST: a prefix entry of 2 x 500 x 200 at reach 2 / 5 with log(tiny) outside the band,
where the weight inside the band underflows float32 and a state lives on the background alone; 1.71 with -inf and 1.68 with
-3 outside on the same shape, 0.88 at 2 x 64 x 1440, at most 0.45 on every other shape; ENTROPY.md, "Band route", has the
table).  Ten times that, rounded to one digit, is 40 units: above the dense route's 20, so the band route asserts its own
4e-5 |ref| + 4e-5 F.  The log-likelihood is held to POSTERIOR.md's bound.  Each test prints the figures it measured."""
import math

import numpy as np
import pytest
import torch

from torbi_amd import entropy, inputs, viterbi

import operand_form_cases as ofc
import path_entropy_band_cases as pbc
import path_entropy_cases as pec
import stream_band_cases as sbc
from workspace_cases import DEV, assert_guards_intact, assert_same_bits, guarded

pytestmark = pytest.mark.gpu

UNIT = 1e-6
MEASURED_WORST = 3.72                    # units, on one MI355X
RTOL_H, ATOL_H_PER_FRAME = 4e-5, 4e-5    # 40 units: ten times MEASURED_WORST, rounded to one digit
DENSE_UNITS = 20.                        # tests/test_path_entropy_gpu.py's bound of the dense route: 2e-5, 2e-5
# (B, T, S, reach_left, reach_right)
SHAPES = ([(3, 4, 5, 10, 10)]                                            # fewer states than a wave, reaches clamped to S - 1
          + [(5, 3, 64, left, right) for left, right in sbc.REACHES]     # one wave, every reach, 0 / 0 and 31 / 31 among them
          + [(4, 2, 65, 2, 5), (2, 3, 1441, 11, 11)]                     # odd states
          + [(2, 3, 1025, 11, 11), (2, 64, 1440, 11, 11)]                # a second state per thread; 64 frames
          + [(5, 1, 64, 3, 2), (1, 1, 65, 2, 2)]                         # one frame
          + [(3, 3, 64, 2, 2), (4, 3, 64, 2, 2), (7, 3, 70, 3, 0)]       # G = 1: several workgroups
          + [(520, 2, 64, 2, 2)]                                         # G = 2
          + [(1023, 3, 64, 3, 2), (1024, 2, 64, 3, 2), (1025, 3, 64, 2, 5)]  # G = 4: a last tile of G - 1, G and 1 items
          + [(2, 500, 200, 2, 5)])                                       # the long one


def device(obs, frames, A, pi, left, right, background, workspace=None, prefix=True):
    out = entropy.forward_entropy_banded(*pec.tensors(obs, frames, A, pi, device=DEV), left, right, float(background),
                                         workspace=workspace, prefix=prefix)
    torch.cuda.synchronize()
    return out


def dense(obs, frames, A, pi):
    out = entropy.forward_entropy(*pec.tensors(obs, frames, A, pi, device=DEV), prefix=True)
    torch.cuda.synchronize()
    return out


def host_copy(out):
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def check(got, want, frames, what, scale=1., scale_l=1.):
    """(entropy, log-likelihood, prefix) of the device within `scale` times the bound on H and the prefix entries and
    `scale_l` times the bound on L of the float64 `want`; prints the worst errors, those of H and the prefix also in units
    of 1e-6 |ref| + 1e-6 F, and returns the latter two."""
    H, L, prefix = pec.numpy(got)
    assert all(x.dtype == torch.float32 and x.device == DEV for x in got)
    T = prefix.shape[1]
    F = pec.clamp(frames, T).astype(np.float64)
    upto = np.minimum(np.arange(1, T + 1, dtype=np.float64)[None, :], F[:, None])
    valid = np.arange(T)[None, :] < F[:, None]
    with np.errstate(invalid='ignore'):
        units = (float(np.nanmax(np.abs(H - want[0]) / (UNIT * np.abs(want[0]) + UNIT * F), initial=0.)),
                 float(np.nanmax((np.abs(prefix - want[2]) / (UNIT * np.abs(want[2]) + UNIT * upto))[valid], initial=0.)))
    print(f'{what}: error of entropy {units[0]:.2f} units, of any prefix entry {units[1]:.2f} units')
    worst = (pec.close(H, want[0], scale * (RTOL_H * np.abs(want[0]) + ATOL_H_PER_FRAME * F), (what, 'entropy')),
             pec.close(prefix, want[2], scale * (RTOL_H * np.abs(want[2]) + ATOL_H_PER_FRAME * upto), (what, 'prefix')),
             pec.close(L, want[1], scale_l * pec.likelihood_bound(want[1], frames, T), (what, 'log-likelihood')))
    assert (prefix[~valid] == 0).all(), (what, 'prefix entries t >= F are 0')
    print(f'{what}: worst error of entropy {worst[0]:.3e}, prefix {worst[1]:.3e}, log-likelihood {worst[2]:.3e}')
    return units


def test_the_shapes_cross_every_edge_of_the_kernel():
    rule = {shape: pbc.items_per_workgroup(shape[0], *shape[2:]) for shape in SHAPES}
    assert (3, 4, 5, 10, 10) in SHAPES and pbc.clamp_reach(10, 5) == 4
    assert {(left, right) for _, _, S, left, right in SHAPES if S == 64} >= set(sbc.REACHES) >= {(0, 0), (31, 31)}
    assert {65, 1441, 1025, 1440} <= {S for _, _, S, _, _ in SHAPES}
    assert (2, 3, 1025, 11, 11) in SHAPES and (2, 64, 1440, 11, 11) in SHAPES and pbc.THREADS < 1025
    assert {1, 2, 3, 64} <= {T for _, T, *_ in SHAPES} and (2, 500, 200, 2, 5) in SHAPES
    if pbc._lib.load().torbi_hip_compute_units(0) == 256:
        assert set(rule.values()) == {1, 2, pbc.MAX_GROUP}
        last = {B % pbc.MAX_GROUP for (B, *_), G in rule.items() if G == pbc.MAX_GROUP}
        assert last == {pbc.MAX_GROUP - 1, 0, 1}                         # G - 1, G and G + 1 items fill the last tiles
    assert sum(1 for (B, *_), G in rule.items() if G == 1 and B > 1) >= 3
    assert {pbc.MAX_GROUP - 1, pbc.MAX_GROUP, pbc.MAX_GROUP + 1} <= {B for B, *_ in SHAPES}


@pytest.mark.parametrize('background', list(pbc.BACKGROUNDS))
@pytest.mark.parametrize('B,T,S,left,right', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_device_against_float64_on_the_full_matrix(B, T, S, left, right, background):
    obs, frames, A, pi = pbc.case(B, T, S, left, right, background, 7 * S + T)
    assert frames[0] == T and (B < 2 or frames[-1] == 1)
    bg = pbc.BACKGROUNDS[background]
    got = device(obs, frames, A, pi, left, right, bg)
    assert got[0].shape == got[1].shape == (B,) and got[2].shape == (B, T)
    check(got, pbc.host64(obs, frames, A, pi), frames, (B, T, S, left, right, background))
    short = device(obs, frames, A, pi, left, right, bg, prefix=False)
    assert len(short) == 2
    assert_same_bits(host_copy(short), host_copy(got[:2]), 'without the prefix output')


@pytest.mark.parametrize('background', list(pbc.BACKGROUNDS))
@pytest.mark.parametrize('B,T,S,left,right', [(5, 3, 64, 2, 5), (4, 2, 65, 2, 5), (2, 64, 1440, 11, 11), (2, 500, 200, 2, 5)])
def test_the_band_route_agrees_with_the_dense_device_route(B, T, S, left, right, background):
    """Each is within its bound of float64, so they are within the sum of the two bounds of each other."""
    obs, frames, A, pi = pbc.case(B, T, S, left, right, background, 7 * S + T)
    got = device(obs, frames, A, pi, left, right, pbc.BACKGROUNDS[background])
    want = pec.numpy(dense(obs, frames, A, pi))
    both = (DENSE_UNITS * UNIT + RTOL_H) / RTOL_H
    check(got, want, frames, ('against the dense device route', B, T, S, background), scale=both, scale_l=2.)


def test_an_item_alone_has_the_bits_it_has_inside_a_batch_of_nan():
    B, T, S, left, right = 2100, 3, 64, 3, 2
    assert pbc.items_per_workgroup(B, S, left, right) in (pbc.MAX_GROUP, 2) and pbc.items_per_workgroup(1, S, left, right) == 1
    for background in ('minus_inf', 'minus_3'):
        bg = pbc.BACKGROUNDS[background]
        obs, _, A, pi = pbc.case(1, T, S, left, right, background, 13)
        alone = host_copy(device(obs, [T], A, pi, left, right, bg))
        assert torch.isfinite(alone[0]).all()
        batch = np.full((B, T, S), np.nan, np.float32)
        at = (0, 1027, 2098)                                             # three workgroups, three places in a tile
        for b in at:
            batch[b] = obs[0]
        H, L, prefix = host_copy(device(batch, [T] * B, A, pi, left, right, bg))
        for b in at:
            assert_same_bits((H[b:b + 1], L[b:b + 1], prefix[b:b + 1]), alone, (background, b))
        others = np.setdiff1d(np.arange(B), at)
        assert torch.isnan(H[others]).all() and torch.isnan(L[others]).all() and torch.isnan(prefix[others]).all()


@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny'])
def test_a_broken_promise_gives_every_item_nan(background):
    """One stray entry outside the band: every item, the one of a single frame included, has NaN in H, L and its prefix
    entries t < F, 0 beyond; nothing raises."""
    B, T, S, left, right = 4, 5, 68, 3, 2
    bg = pbc.BACKGROUNDS[background]
    obs, _, A, pi = pbc.case(B, T, S, left, right, background, 21)
    frames = np.array([5, 3, 1, 4], np.int32)
    strays = [(40, 3, np.float32(-1.))] + ([(40, 3, -A[40, 3])] if background == 'log_tiny' else [])     # (the sign bit alone)
    for j, i, value in strays:
        stray = np.array(A)
        stray[j, i] = value
        H, L, prefix = host_copy(device(obs, frames, stray, pi, left, right, bg))
        assert torch.isnan(H).all() and torch.isnan(L).all()
        for b in range(B):
            f = int(frames[b])
            assert torch.isnan(prefix[b, :f]).all() and (prefix[b, f:] == 0).all(), b


@pytest.mark.parametrize('background', ['minus_inf', 'minus_3'])
@pytest.mark.parametrize('value', [math.nan, math.inf])
@pytest.mark.parametrize('where', ['observation', 'observation_beyond', 'initial', 'matrix'])
def test_non_finite_rule(where, value, background):
    B, T, S, left, right = 4, 5, 70, 3, 2
    bg = pbc.BACKGROUNDS[background]
    obs, _, A, pi = pbc.case(B, T, S, left, right, background, 21)
    frames = np.array([5, 3, 1, 4], np.int32)
    clean = host_copy(device(obs, frames, A, pi, left, right, bg))
    assert all(torch.isfinite(x).all() for x in clean)
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
    H, L, prefix = host_copy(device(obs, frames, A, pi, left, right, bg))
    for b in range(B):
        f = int(frames[b])
        if b in bad:
            assert torch.isnan(H[b]) and torch.isnan(L[b]) and torch.isnan(prefix[b, :f]).all() and (prefix[b, f:] == 0).all()
        else:                                                    # the neighbours' bits do not change
            assert_same_bits((H[b:b + 1], L[b:b + 1], prefix[b]), (clean[0][b:b + 1], clean[1][b:b + 1], clean[2][b]), (where, b))


@pytest.mark.parametrize('background', ['minus_inf', 'minus_3'])
def test_an_item_of_total_probability_zero(background):
    B, T, S, left, right = 3, 4, 70, 3, 2
    bg = pbc.BACKGROUNDS[background]
    obs, _, A, pi = pbc.case(B, T, S, left, right, background, 3)
    frames = np.array([4, 4, 2], np.int32)
    clean = host_copy(device(obs, frames, A, pi, left, right, bg))
    obs = np.array(obs)
    obs[1, 2, :] = -np.inf                                       # no state can emit frame 2 of item 1
    H, L, prefix = host_copy(device(obs, frames, A, pi, left, right, bg))
    assert L[1] == -math.inf and torch.isnan(H[1]) and torch.isnan(prefix[1]).all()
    for b in (0, 2):
        assert_same_bits((H[b:b + 1], L[b:b + 1], prefix[b]), (clean[0][b:b + 1], clean[1][b:b + 1], clean[2][b]), b)


@pytest.mark.parametrize('background', list(pbc.BACKGROUNDS))
@pytest.mark.parametrize('B,T,S', [(5, 6, 70), (3, 50, 200)])
def test_minus_inf_cells_inside_the_band_make_no_nan(B, T, S, background):
    """Left to right inside the band: the in-band cells with prev > next are -inf (G is 0 there, 0 x -inf is never formed)."""
    left, right = 3, 2
    bg = pbc.BACKGROUNDS[background]
    obs, frames, A, pi = pbc.case(B, T, S, left, right, background, 7 * S + T, True)
    j, i = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    assert np.isneginf(A[(i > j) & (i <= j + right)]).all() and np.isfinite(A[(i <= j) & (i >= j - left)]).all()
    got = device(obs, frames, A, pi, left, right, bg)
    assert not any(torch.isnan(x).any() for x in got)
    check(got, pbc.host64(obs, frames, A, pi), frames, ('left to right inside the band', B, T, S, background))


def test_a_state_no_path_reaches_contributes_nothing_and_makes_no_nan():
    B, T, S, left, right = 5, 6, 70, 3, 2
    obs, frames, A, _ = pbc.case(B, T, S, left, right, 'minus_inf', 5, True)
    start = np.full((S,), -np.inf, np.float32)
    start[10] = -0.5                                             # every path starts in state 10 and never goes below it
    got = device(obs, frames, A, start, left, right, -np.inf)
    assert not any(torch.isnan(x).any() for x in got)
    want = pbc.host64(obs, frames, A, start)
    assert (want[2][:, 0] == 0).all()                            # one state at frame 0: this route gives 0 within the bound
    check(got, want, frames, 'left to right from one state')


# ------------------------------------------------------------------------------------------------ the caller's workspace
WORKSPACE_CASES = {'minus_inf-9x6x68': (9, 6, 68, 3, 2, 'minus_inf'), 'minus_3-5x4x130': (5, 4, 130, 31, 31, 'minus_3'),
                   'log_tiny-3x5x1025': (3, 5, 1025, 2, 5, 'log_tiny')}


@pytest.mark.parametrize('name', list(WORKSPACE_CASES))
def test_workspace_contract(name):
    """Exactly the queried bytes, at a 256-byte aligned base and one byte past it (the layout rounds the base up, so both are
    taken); over 0x00 and 0xFF; with and without the prefix output; after a call whose inputs are NaN and after a broken
    promise; a byte short raises before anything is launched."""
    B, T, S, left, right, background = WORKSPACE_CASES[name]
    bg = pbc.BACKGROUNDS[background]
    obs, frames, A, pi = pbc.case(B, T, S, left, right, background, 7 * S + T)
    need = entropy.path_entropy_banded_workspace_bytes(B, T, S, left, right)
    fresh = host_copy(device(obs, frames, A, pi, left, right, bg))
    check(device(obs, frames, A, pi, left, right, bg), pbc.host64(obs, frames, A, pi), frames, name)
    for offset, fill in ((0, 0xC3), (1, 0x00), (1, 0xFF)):
        for prefix in (True, False):
            ws = guarded(need, offset=offset, fill=fill)
            got = host_copy(device(obs, frames, A, pi, left, right, bg, workspace=ws, prefix=prefix))
            assert_same_bits(got, fresh[:len(got)], (name, offset, fill, prefix))
            assert_guards_intact(ws)
    ws = guarded(need, offset=1, fill=0xFF)
    dirty_obs, dirty_pi = np.array(obs), np.full_like(pi, np.nan)
    dirty_obs[0, min(1, T - 1), 5] = np.nan
    flagged = host_copy(device(dirty_obs, frames, A, dirty_pi, left, right, bg, workspace=ws))
    assert torch.isnan(flagged[0]).all() and torch.isnan(flagged[1]).all()
    assert_same_bits(host_copy(device(obs, frames, A, pi, left, right, bg, workspace=ws)), fresh, (name, 'after a call that left NaN behind'))
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
    H, L, prefix = entropy.forward_entropy_banded(torch.empty(0, 3, 64, device=DEV), None, A, torch.zeros(64, device=DEV), 2, 2,
                                                  prefix=True)
    assert H.shape == L.shape == (0,) and prefix.shape == (0, 3) and H.device == DEV
    assert len(entropy.forward_entropy_banded(torch.empty(0, 3, 64, device=DEV), None, A, torch.zeros(64, device=DEV), 2, 2)) == 2


# ------------------------------------------------------------------------------------------------ graphs and streams
@pytest.mark.parametrize('background', ['minus_inf', 'minus_3'])
def test_graph_capture_and_two_replays_on_new_observations(background):
    B, T, S, left, right = 5, 7, 68, 3, 2
    bg = float(pbc.BACKGROUNDS[background])
    first, frames, A, pi = pbc.case(B, T, S, left, right, background, 31)
    obs, f, A_, pi_ = pec.tensors(first, frames, A, pi, device=DEV)
    ws = torch.empty(entropy.path_entropy_banded_workspace_bytes(B, T, S, left, right), dtype=torch.uint8, device=DEV)
    entropy.forward_entropy_banded(obs, f, A_, pi_, left, right, bg, workspace=ws, prefix=True)     # (loads the kernels outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = entropy.forward_entropy_banded(obs, f, A_, pi_, left, right, bg, workspace=ws, prefix=True)
    for seed in (32, 33):
        again = pbc.case(B, T, S, left, right, background, seed)[0]
        obs.copy_(torch.from_numpy(again))
        graph.replay()
        torch.cuda.synchronize()
        want = entropy.forward_entropy_banded(obs.clone(), f, A_, pi_, left, right, bg, prefix=True)
        assert_same_bits(host_copy(out), host_copy(want), 'a replayed graph against a fresh call')
        check(out, pbc.host64(again, frames, A, pi), frames, ('replay', seed))


def test_a_call_on_another_stream():
    B, T, S, left, right = 5, 7, 68, 3, 2
    obs, frames, A, pi = pbc.case(B, T, S, left, right, 'minus_3', 31)
    ops = pec.tensors(obs, frames, A, pi, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = entropy.forward_entropy_banded(*ops, left, right, -3., prefix=True)
    stream.synchronize()
    check(out, pbc.host64(obs, frames, A, pi), frames, 'another stream')


# ------------------------------------------------------------------------------------------------ the front
def test_path_entropy_band_takes_probabilities_and_writes_nothing():
    B, T, S, left, right = 9, 6, 68, 3, 2
    g = torch.Generator().manual_seed(3)
    obs = torch.softmax(3 * torch.randn(B, T, S, generator=g), 2)
    A = torch.exp(torch.from_numpy(sbc.band_matrix(S, left, right, -np.inf, seed=4)))
    pi = torch.softmax(torch.randn(S, generator=g), 0)
    frames = torch.from_numpy(pec.ragged(B, T, 3))
    before, matrix = obs.clone(), A.clone()
    got = entropy.path_entropy(obs, frames, A, pi, gpu=0, prefix=True, route='band')
    assert torch.equal(obs, before) and torch.equal(A, matrix)
    assert len(entropy.path_entropy(obs, frames, A, pi, gpu=0, route='band')) == 2
    # the same call by hand: the prepared inputs, the band the look finds, the operator
    trans, uniform, init = inputs.model(A, pi, False, S, DEV, plain=True)
    band = viterbi.band_over(trans, trans, S)
    assert uniform is None and band is not None and tuple(band[:2]) == (left, right)
    by_hand = entropy.forward_entropy_banded(inputs.observation(obs, False, DEV), frames, trans, init, *band, prefix=True)
    assert_same_bits(host_copy(got), host_copy(by_hand), "path_entropy(route='band') against forward_entropy_banded")
    want = entropy.path_entropy(obs, frames, A, pi, gpu=None, prefix=True)
    check(got, tuple(x.double().numpy() for x in want), frames.numpy(), "path_entropy(route='band')")
    # 'auto' takes what `path_entropy_route` says
    said = entropy.path_entropy_route(A, B, T, S, gpu=0)
    assert said == ('band' if entropy._band_pays(B, S, left, right) else 'dense')
    auto = host_copy(entropy.path_entropy(obs, frames, A, pi, gpu=0, prefix=True, route='auto'))
    same_as = host_copy(entropy.path_entropy(obs, frames, A, pi, gpu=0, prefix=True, route=said))
    assert_same_bits(auto, same_as, "route='auto' against route=" + said)
    assert_same_bits(host_copy(entropy.path_entropy(obs, frames, A, pi, gpu=0, prefix=True)),
                     host_copy(entropy.path_entropy(obs, frames, A, pi, gpu=0, prefix=True, route='dense')), 'the default is dense')


def test_band_raises_with_the_planner_s_reason_where_there_is_no_covered_band():
    B, T, S = 3, 4, 70                                           # 70 % 4 != 0: viterbi.band_over cannot answer
    obs, frames, A, pi = pbc.case(B, T, S, 2, 1, 'minus_inf', 5)
    o, f, a, p = pec.tensors(obs, frames, A, pi)
    with pytest.raises(RuntimeError) as raised:
        entropy.path_entropy(o, f, a, p, log_probs=True, gpu=0, route='band')
    assert str(raised.value).startswith("path_entropy(route='band'): the matrix does not hold one value outside a band")
    assert entropy.path_entropy_route(a, B, T, S, gpu=0, log_probs=True) == 'dense'
    assert_same_bits(host_copy(entropy.path_entropy(o, f, a, p, log_probs=True, gpu=0, route='auto')),
                     host_copy(entropy.path_entropy(o, f, a, p, log_probs=True, gpu=0, route='dense')), 'auto without a band')


# ------------------------------------------------------------------------------------------------ operand forms
FORM_CASES = pbc.form_cases(DEV)


@pytest.mark.parametrize('name,operand,form_name', FORM_CASES, ids=['-'.join(c) for c in FORM_CASES])
def test_a_form_equals_its_plain_copy_and_nothing_is_written(name, operand, form_name):
    ofc.check_forms(pbc.ENTRY[name], DEV, 0, {operand: form_name})


@pytest.mark.parametrize('name', list(pbc.ENTRY))
def test_every_operand_in_another_form_at_once(name):
    entry = pbc.ENTRY[name]
    ofc.check_forms(entry, DEV, 0, {operand: ofc.TOGETHER[operand] for operand in entry.operands})
