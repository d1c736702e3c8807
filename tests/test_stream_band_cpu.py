"""The band route of torbi_amd.StreamDecoder, as far as it goes without a device: the prefix / band / suffix rule of
csrc/stream_band.hpp restated in numpy (tests/stream_band_cases.py) against the full-row rule of tests/stream_cases.py, bit
for bit; that the tie inputs tie where the rule can go wrong; and the surface -- signature, exports, header, symbol table,
`covers` and the argument checks of the C entry points, none of which touches a device."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, synth
from stream_cases import clamp, plan, feed, reference_arrays, reference_path
from stream_band_cases import (BACKGROUNDS, REACHES, band_arrays, band_matrix, continuous, dead_initial, diagonals, grid_scores,
                               nonfinite_sources, tie_background, tie_counts, tie_problem)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, T = 64, 24
BAND_SYMBOLS = ['torbi_hip_stream_band_covers', 'torbi_hip_stream_band_tile', 'torbi_hip_stream_band_diagonals_bytes',
                'torbi_hip_stream_band_prepare', 'torbi_hip_stream_band_push', 'torbi_hip_stream_band_flush']


def same_arrays(seq, trans, init, reach_left, reach_right, background):
    """band_arrays == reference_arrays: rows (NaN positions included) and pointers, bit for bit."""
    with np.errstate(invalid='ignore'):
        post, bp = reference_arrays(seq, trans, init)
    got_post, got_bp = band_arrays(seq, diagonals(trans, reach_left, reach_right), reach_left, reach_right, background, init)
    assert np.array_equal(np.isnan(got_post), np.isnan(post))
    assert np.array_equal(got_post.view(np.int32)[~np.isnan(post)], post.view(np.int32)[~np.isnan(post)])
    assert np.array_equal(got_bp, bp)
    return post, bp


def families(seed):
    """(name, sequences, initial or None) of every input family of the GPU file."""
    dead = continuous(2, T, S, seed + 5)
    dead[1, 0, 0] = np.inf
    spot = continuous(1, T, S, seed + 6)
    spot[0, 0, 5] = np.inf
    return [('continuous', list(continuous(2, T, S, seed)), None),
            ('zeros', [np.zeros((T, S), np.float32)], np.zeros(S, np.float32)),
            ('grid4', list(grid_scores(2, T, S, 4, seed + 1)), np.zeros(S, np.float32)),
            ('grid7', list(grid_scores(2, T, S, 7, seed + 2)), np.zeros(S, np.float32)),
            ('nonfinite', nonfinite_sources(T, S, seed + 3), None),
            ('dead', [dead[0]], dead_initial(S)),
            ('dead-inf-at-0', [dead[1]], dead_initial(S, plus_inf_at=0)),
            ('dead-inf-at-5', [spot[0]], dead_initial(S, plus_inf_at=5))]


# ------------------------------------------------------------------------------------------------------ 1: the rule
@pytest.mark.parametrize('background', list(BACKGROUNDS))
@pytest.mark.parametrize('reach', REACHES, ids=[f'{a}-{b}' for a, b in REACHES])
def test_band_rule_is_the_full_row_rule(reach, background):
    """Every input family x continuous and grid-valued in-band scores: rows, pointers and NaN positions."""
    left, right = reach
    bg = BACKGROUNDS[background]
    seed = 100 * left + right
    flat = synth.problem(1, 1, S, seed=seed)[2]
    seen_nan = seen_dead = 0
    for grid in (None, 8):
        trans = band_matrix(S, left, right, bg, seed=seed, grid=grid)
        for name, sequences, init in families(seed):
            for seq in sequences:
                post, bp = same_arrays(seq, trans, flat if init is None else init, left, right, bg)
                seen_nan += int(np.isnan(post).any())
                seen_dead += int(np.isneginf(post[-1]).all())
    assert seen_nan >= 4 and seen_dead >= 2                  # the non-finite families did what they are for


def test_zero_matrix_with_zero_background_points_at_state_0():
    """All-zero scores: every candidate ties, wherever the band ends."""
    zeros = np.zeros((T, S), np.float32)
    for left, right in REACHES:
        _, bp = same_arrays(zeros, np.zeros((S, S), np.float32), np.zeros(S, np.float32), left, right, 0.)
        assert (bp == 0).all()


def test_first_non_nan_candidate_of_a_dead_row():
    """A row of -inf with one +inf beside a -inf background: a state whose band misses the +inf has a NaN candidate there,
    which is skipped, and points at the first candidate that is not NaN; c_0 = NaN gives NaN and pointer 0."""
    left, right = 2, 2
    trans = band_matrix(S, left, right, -np.inf, seed=1)
    seq = continuous(1, 3, S, 2)[0]
    for at in (0, 5):
        seq0 = seq.copy()
        seq0[0, at] = np.inf
        post, bp = same_arrays(seq0, trans, dead_initial(S, plus_inf_at=at), left, right, -np.inf)
        assert np.isposinf(post[0, at]) and np.isneginf(np.delete(post[0], at)).all()
        far = [j for j in range(S) if not at - right <= j <= at + left]           # states whose band misses `at`
        if at == 0:
            assert np.isnan(post[1, far]).all() and (bp[1, far] == 0).all()
        else:
            assert np.isneginf(post[1, far]).all() and (bp[1, far] == 0).all()
            assert (bp[1, at - right:at + left + 1] == at).all()


# ------------------------------------------------------------------------------------------------------ 2: the ties tie
@pytest.mark.parametrize('reach', [(2, 2), (0, 3), (3, 0), (2, 5), (5, 2), (31, 31)], ids=lambda r: f'{r[0]}-{r[1]}')
def test_tie_inputs_tie_on_both_sides_of_the_band(reach):
    """On the numpy reference: frames where a candidate left of the band equals the in-band best (the prefix must win) and
    where the in-band best equals a candidate right of it (the band must win); then the band rule on that input."""
    left, right = reach
    obs, trans, init = tie_problem(S, left, right, seed=7 + left)
    prefix_wins, band_wins = tie_counts(obs, trans, init, left, right, reference_arrays)
    print(f'reach {left}/{right}: the prefix must win {prefix_wins} times, the band {band_wins} times')
    assert prefix_wins > 0 and band_wins > 0, (prefix_wins, band_wins)
    same_arrays(obs, trans, init, left, right, tie_background(left, right))


# ------------------------------------------------------------------------------------------------------ 3: surface
def test_route_is_an_argument_and_stream_route_is_exported():
    assert inspect.signature(torbi_amd.StreamDecoder.__init__).parameters['route'].default == 'auto'
    assert 'stream_route' in torbi_amd.__all__ and callable(torbi_amd.stream_route)
    assert torbi_amd.stream_route(None, 2, 64, gpu=None) == 'host'


@pytest.mark.parametrize('gpu', [None])
def test_route_bogus_raises(gpu):
    with pytest.raises(ValueError):
        torbi_amd.StreamDecoder(2, 64, gpu=gpu, route='bogus')


@pytest.mark.parametrize('route', ['auto', 'dense', 'band'])
def test_host_decoder_ignores_the_route(route):
    B, frames = 2, 20
    obs = continuous(B, frames, S, 11)
    trans, init = band_matrix(S, 2, 2, -np.inf, seed=3), np.zeros(S, np.float32)
    dec = torbi_amd.StreamDecoder(B, S, torch.from_numpy(trans), torch.from_numpy(init), log_probs=True, gpu=None, route=route)
    assert dec.route == 'host'
    got, _ = feed(dec, [obs[b] for b in range(B)], plan(B, frames, 'ragged', seed=1))
    for b in range(B):
        assert np.array_equal(got[b], reference_path(clamp(obs[b]), trans, init))


def test_header_and_symbol_table_declare_the_band_entries():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    for name in BAND_SYMBOLS:
        assert re.search(r'\b(?:int|size_t) ' + name + r'\s*\(', header), name
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    push = re.search(r'int torbi_hip_stream_band_push\s*\(([^;]*)\);', header).group(1)
    assert re.search(r'int32_t \*counts_out, int max_lag, int32_t \*forced_out,\s*int B, int S, int device, void \*stream', push)
    assert _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert re.search(r'#define TORBI_HIP_ABI_VERSION 17\b', header)


def test_covers_answers_without_a_device():
    covers = _lib.load().torbi_hip_stream_band_covers
    f = ctypes.c_float
    for bg in (-math.inf, float(BACKGROUNDS['log_tiny']), -20.):
        assert covers(1, 1440, 87, 87, f(bg), 0) == 1 and covers(512, 1440, 11, 11, f(bg), 0) == 1
        assert covers(1, 64, 0, 0, f(bg), 0) == 1 and covers(1, 3072, 254, 254, f(bg), 0) == 1
    assert covers(1, 1440, 87, 87, f(math.nan), 0) == 0 and covers(1, 1440, 87, 87, f(math.inf), 0) == 0
    for states in (1438, 1441, 66, 60, 3076):
        assert covers(1, states, 2, 2, f(-math.inf), 0) == 0, states
    assert covers(1, 1440, 254, 255, f(0.), 0) == 0 and covers(1, 1440, -1, 2, f(0.), 0) == 0 and covers(0, 1440, 2, 2, f(0.), 0) == 0
    tile = _lib.load().torbi_hip_stream_band_tile
    assert tile(1, 1440, 87, 87, 0) == 1 and tile(1, 1442, 87, 87, 0) == -5 and tile(0, 1440, 87, 87, 0) == -1
    assert _lib.load().torbi_hip_stream_band_diagonals_bytes(1440, 87, 87) == 175 * 1440 * 4


def test_band_entries_answer_bad_arguments_before_any_device_work():
    """push, flush and prepare with host pointers nobody reads: every call is turned down by its arguments."""
    lib = _lib.load()
    EINVAL, EWORKSPACE, ERANGE, EUNSUPPORTED = -1, -2, -3, -5
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, states, cap, out_cap = 3, 64, 4, 6
    need = lib.torbi_hip_stream_state_bytes(B, states, cap)

    def push(lag=-1, forced=null, obs=p, Tc=2, info=p, diag=p, init=p, left=2, right=2, bg=-math.inf, state=p, nbytes=need,
             cap=cap, out=p, out_cap=out_cap, counts=p, B=B, S=states):
        return lib.torbi_hip_stream_band_push(obs, Tc, info, diag, init, left, right, ctypes.c_float(bg), state, nbytes, cap, out,
                                              out_cap, counts, lag, forced, B, S, 0, null)

    def flush(info=p, state=p, nbytes=need, cap=cap, out=p, out_cap=out_cap, counts=p, B=B, S=states):
        return lib.torbi_hip_stream_band_flush(info, state, nbytes, cap, out, out_cap, counts, B, S, 0, null)

    for name in ('info', 'state', 'out', 'counts'):
        assert push(**{name: null}) == EINVAL and flush(**{name: null}) == EINVAL, name
    for name in ('B', 'S', 'cap', 'out_cap'):
        for value in (0, -1):
            assert push(**{name: value}) == EINVAL and flush(**{name: value}) == EINVAL, (name, value)
    assert push(diag=null) == EINVAL and push(obs=null) == EINVAL and push(init=null) == EINVAL and push(Tc=-1) == EINVAL
    assert push(nbytes=need - 1) == EWORKSPACE and flush(nbytes=need - 1) == EWORKSPACE and push(cap=cap + 1) == EWORKSPACE
    assert push(S=8001, nbytes=1 << 40) == ERANGE and flush(S=8001, nbytes=1 << 40) == ERANGE
    assert push(lag=-2) == EINVAL and push(lag=0) == EINVAL and push(lag=7) == EINVAL          # a bound without forced_out
    assert push(left=-1) == EINVAL and push(right=-1) == EINVAL
    big = lib.torbi_hip_stream_state_bytes(B, 4000, cap)
    for kwargs in (dict(S=66, nbytes=big), dict(S=60, nbytes=big), dict(S=3076, nbytes=big), dict(left=300, right=300),
                   dict(bg=math.nan), dict(bg=math.inf)):
        assert push(**kwargs) == EUNSUPPORTED and push(lag=3, forced=p, **kwargs) == EUNSUPPORTED, kwargs
    assert flush(S=66, nbytes=big) == EUNSUPPORTED and flush(S=3076, nbytes=big) == EUNSUPPORTED

    def prepare(trans=p, S=states, left=2, right=2, bg=-math.inf, diag=p, ok=p):
        return lib.torbi_hip_stream_band_prepare(trans, S, left, right, ctypes.c_float(bg), diag, ok, 0, null)
    for name in ('trans', 'diag', 'ok'):
        assert prepare(**{name: null}) == EINVAL, name
    assert prepare(S=0) == EINVAL and prepare(left=-1) == EINVAL and prepare(right=-1) == EINVAL
    assert prepare(S=66) == EUNSUPPORTED and prepare(bg=math.nan) == EUNSUPPORTED and prepare(left=300, right=300) == EUNSUPPORTED
