"""The wide band route of path entropy on an MI355X (csrc/path_entropy_wide_band.hpp behind torbi_hip_path_entropy_wide_band,
entropy.forward_entropy_wide_banded and the routing of entropy.path_entropy) against the float64 host route on the FULL
matrix (`entropy._host`), on entropy, every prefix entry and the log-likelihood.

The bound is the narrow band route's, asserted by its own `check` (tests/test_path_entropy_band_gpu.py): 4e-5 |ref| + 4e-5 F
on H and on prefix_t (F = t + 1), `pec.likelihood_bound` on L.  `check` prints the worst error of every case in units of
1e-6 |ref| + 1e-6 F; ENTROPY.md, "Wide band route", has the table.

pe_wide_band_kernel<G> is instantiated for G = 1 and 2 (4 needs scratch).  On 256 compute units a batch below 511 items runs
G = 1 and 515 items run G = 2 with a last tile of one item."""
import numpy as np
import pytest
import torch

from torbi_amd import _lib, entropy, inputs, viterbi

import path_entropy_band_cases as pbc
import path_entropy_cases as pec
from test_path_entropy_band_gpu import check, host_copy
from workspace_cases import DEV, assert_guards_intact, assert_same_bits, guarded

pytestmark = pytest.mark.gpu

# B, T, S, reach_left, reach_right, background, left to right inside the band
CASES = [(1, 1, 8, 7, 7, 'minus_inf', False),              # one frame reads no matrix entry; the band clipped to the matrix
         (3, 12, 72, 40, 30, 'minus_inf', False),          # just past 64 entries, asymmetric, S no multiple of 64
         (3, 12, 72, 30, 40, 'minus_3', False),            # a finite background: all three constants
         (2, 9, 131, 130, 130, 'log_tiny', False),         # the band is the whole matrix; odd S, a ragged last quad of states
         (2, 8, 1440, 87, 87, 'minus_inf', False),         # the pitch shape: 6 blocks x 2 slices
         (2, 8, 1440, 87, 87, 'log_tiny', False),
         (2, 4, 4096, 255, 256, 'minus_inf', False),       # the widest band, the most states, 1 slice
         (2, 500, 200, 40, 30, 'log_tiny', False),         # the long one: the narrow route's worst case, widened
         (3, 12, 72, 40, 30, 'minus_inf', True),           # -inf cells inside the band
         (3, 3, 68, 40, 33, 'minus_inf', False),           # G = 1
         (515, 3, 68, 40, 33, 'minus_inf', False)]         # G = 2, the largest tile, and a partial last one
TILES = {3: 1, 515: 2}                                     # the G rule at 256 compute units


def problem(case):
    B, T, S, left, right, background, left_to_right = case
    return pbc.case(B, T, S, left, right, background, 7 * S + T, left_to_right)


def wide(obs, frames, A, pi, case, workspace=None, prefix=True):
    out = entropy.forward_entropy_wide_banded(*pec.tensors(obs, frames, A, pi, device=DEV), case[3], case[4],
                                              float(pbc.BACKGROUNDS[case[5]]), workspace=workspace, prefix=prefix)
    return host_copy(out)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c[:3])) + f'-{c[3]}-{c[4]}-{c[5]}' + '-ltr' * c[6])
def test_against_float64(case):
    B, T, S = case[:3]
    if S == 68 and _lib.load().torbi_hip_compute_units(0) == 256:
        assert _lib.load().torbi_hip_path_entropy_wide_band_tile(B, S, case[3], case[4], 0) == TILES[B]
    obs, frames, A, pi = problem(case)
    got = wide(obs, frames, A, pi, case)
    assert got[0].shape == got[1].shape == (B,) and got[2].shape == (B, T)
    assert not any(torch.isnan(x).any() for x in got)
    check(tuple(x.to(DEV) for x in got), pbc.host64(obs, frames, A, pi), frames, case)
    assert_same_bits(wide(obs, frames, A, pi, case, prefix=False), got[:2], 'without the prefix output')


def test_a_nan_inside_the_band_reaches_exactly_the_items_that_take_a_step():
    case = CASES[1]
    obs, frames, A, pi = problem(case)
    bad = np.array(A)
    bad[20, 50] = np.nan                                                  # next 20, prev 50: inside reach_right = 30
    H, L, prefix = wide(obs, frames, bad, pi, case)
    F = pec.clamp(frames, case[1])
    assert {1} < set(F.tolist())
    for b in range(case[0]):
        hit = bool(F[b] >= 2)
        assert bool(torch.isnan(H[b])) == bool(torch.isnan(L[b])) == hit
        assert bool(torch.isnan(prefix[b, :F[b]]).all()) == hit and (prefix[b, F[b]:] == 0).all()


@pytest.mark.parametrize('case', [CASES[1], CASES[2]], ids=['minus_inf', 'minus_3'])
def test_a_broken_promise_is_nan(case):
    obs, frames, A, pi = problem(case)
    stray = np.array(A)
    stray[60, 3] = -1.0                                                   # outside the stated band, not the background
    H, L, prefix = wide(obs, frames, stray, pi, case)
    F = pec.clamp(frames, case[1])
    assert torch.isnan(H).all() and torch.isnan(L).all()
    assert all(torch.isnan(prefix[b, :F[b]]).all() and (prefix[b, F[b]:] == 0).all() for b in range(case[0]))


def test_an_item_s_bits_depend_neither_on_its_tile_nor_on_the_batch():
    case = CASES[-1]
    obs, frames, A, pi = problem(case)
    whole = wide(obs, frames, A, pi, case)                               # G = 2; item 514 sits alone in the last tile
    for rows in (slice(0, 1), slice(513, 515), slice(1, 4)):               # G = 1: alone, across the last tiles, odd start
        part = wide(obs[rows], frames[rows], A, pi, case)
        assert_same_bits(part, tuple(x[rows] for x in whole), rows)


def test_a_caller_owned_workspace_of_exactly_the_queried_bytes():
    case = CASES[2]
    obs, frames, A, pi = problem(case)
    ws = guarded(entropy.path_entropy_wide_banded_workspace_bytes(*case[:5]), offset=1, fill=0xFF)
    assert_same_bits(wide(obs, frames, A, pi, case, workspace=ws), wide(obs, frames, A, pi, case), 'a stale, odd-based workspace')
    assert_guards_intact(ws)


@pytest.mark.parametrize('left,right,entry', [(40, 30, 'forward_entropy_wide_banded'), (30, 33, 'forward_entropy_banded')])
def test_route_band_of_path_entropy(left, right, entry):
    """`route='band'`: the wide route for a band of 71 entries, the narrow route bit for bit for one of 64; 'auto' takes what
    `path_entropy_route` says."""
    B, T, S = 3, 12, 72
    obs, frames, A, pi = pbc.case(B, T, S, left, right, 'minus_inf', 5)
    o, f, a, p = pec.tensors(obs, frames, A, pi)
    got = entropy.path_entropy(o, f, a, p, log_probs=True, gpu=0, prefix=True, route='band')
    trans, uniform, init = inputs.model(a, p, True, S, DEV, plain=True)
    band = viterbi.band_over(trans, trans, S)
    assert uniform is None and tuple(band[:2]) == (left, right)
    want = getattr(entropy, entry)(inputs.observation(o, True, DEV), f, trans, init, *band, prefix=True)
    assert_same_bits(host_copy(got), host_copy(want), entry)
    assert not torch.isnan(got[1]).any()
    said = entropy.path_entropy_route(a, B, T, S, gpu=0, log_probs=True)
    assert said in ('band', 'dense')
    assert_same_bits(host_copy(entropy.path_entropy(o, f, a, p, log_probs=True, gpu=0, prefix=True, route='auto')),
                     host_copy(entropy.path_entropy(o, f, a, p, log_probs=True, gpu=0, prefix=True, route=said)), said)
