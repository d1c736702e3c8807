"""The band route of torbi_amd.StreamPosteriors without a device: the surface of torbi_hip_stream_smooth_band_* (what it
covers, its tile sizes for 256 compute units, the size of the diagonals, every argument code -- all answered before any
device work) and what the constructor and `stream_posterior_route` do with `route=` and `band=`."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib
from stream_posterior_cases import HOST_GAMMA, Feeder, cpu, problem
from stream_posterior_band_cases import (BACKGROUNDS, EINVAL, ERANGE, EUNSUPPORTED, EWORKSPACE, MAX_STATES, NAMES, TILES, TINY,
                                         band_problem, bits, lds_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. surface --------------------------------------------------------------------------------------------------------

def test_the_six_entries_are_declared_exported_and_bound_within_abi_17():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(?:int|size_t) ' + name + r'\s*\(', header), name
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert not name.endswith('_bytes')
    declared = set(re.findall(r'\b(torbi_hip_stream_smooth_band_\w+)', header))
    assert declared == set(NAMES) == {n for n in _lib.SYMBOLS if n.startswith('torbi_hip_stream_smooth_band_')}
    assert '#define TORBI_HIP_ABI_VERSION 17' in header and _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert 'stream_posterior_route' in torbi_amd.__all__ and callable(torbi_amd.stream_posterior_route)


# ---- 2. coverage -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('background', [-math.inf, TINY, -20.])
def test_covers_takes_what_the_offline_band_route_takes_of_a_matrix(background):
    covers = _lib.load().torbi_hip_stream_smooth_band_covers
    for B, S, left, right in [(1, 1440, 11, 11), (512, 1440, 11, 11), (1, 1, 0, 0), (1, 37, 36, 36), (1, 4096, 31, 32)]:
        assert covers(B, S, left, right, background, -1) == 1, (B, S, left, right)
        # the same answer as the offline route's for a matrix (its T only bounds the grid)
        assert _lib.load().torbi_hip_forward_backward_band_covers(B, 1, S, left, right, background, -1) == 1
    assert covers(1, 37, 1000, 1000, background, -1) == 1          # (the reaches are clamped to S - 1)
    assert covers(1, MAX_STATES + 1, 11, 11, background, -1) == 0
    assert covers(1, 1440, 32, 32, background, -1) == 0             # 65 diagonals
    assert covers(1, 1440, 31, 32, background, -1) == 1
    assert covers(1, 1440, -1, 11, background, -1) == 0 and covers(1, 1440, 11, -1, background, -1) == 0
    assert covers(0, 1440, 11, 11, background, -1) == 0 and covers(1, 0, 0, 0, background, -1) == 0


def test_covers_turns_down_a_nan_or_plus_infinite_background():
    covers = _lib.load().torbi_hip_stream_smooth_band_covers
    assert covers(1, 1440, 11, 11, math.nan, -1) == 0 and covers(1, 1440, 11, 11, math.inf, -1) == 0
    assert covers(1, 1440, 11, 11, 0., -1) == 1 and covers(1, 1440, 11, 11, 5., -1) == 1


def test_the_tile_query_answers_without_a_device_for_256_compute_units():
    tile = _lib.load().torbi_hip_stream_smooth_band_tile
    assert tile(0, 64, 1, 2, -1) == EINVAL and tile(4, 0, 1, 2, -1) == EINVAL and tile(4, 64, -1, 2, -1) == EINVAL
    assert tile(4, 64, 1, -2, -1) == EINVAL
    assert tile(1, MAX_STATES + 1, 1, 2, -1) == EUNSUPPORTED and tile(1, 1440, 32, 32, -1) == EUNSUPPORTED
    # 8, halved while the workgroups are fewer than 256 compute units
    for S in (63, 64):
        for G, B in TILES:
            assert tile(B, S, 1, 2, -1) == G, (S, G, B)
            if G > 1:
                assert tile(B - 1, S, 1, 2, -1) == G // 2, (S, G, B)
        assert tile(1 << 20, S, 1, 2, -1) == 8
    # ... after it was halved while the rows of G streams exceed 64 KB of LDS
    for S, left, right, most in [(1440, 11, 11, 4), (998, 5, 2, 8), (999, 5, 2, 4), (2040, 0, 0, 2), (4096, 31, 32, 1), (37, 36, 36, 8)]:
        assert tile(1 << 20, S, left, right, -1) == most, (S, left, right)
        assert lds_bytes(most, S, left, right) <= 65536 and (most == 8 or lds_bytes(2 * most, S, left, right) > 65536)
    assert [tile(B, 1440, 11, 11, -1) for B in (1, 510, 511, 512, 1020, 1021, 4096)] == [1, 1, 2, 2, 2, 4, 4]


def test_the_diagonals_size_is_both_orders_of_the_clamped_band_and_zero_for_a_bad_argument():
    size = _lib.load().torbi_hip_stream_smooth_band_diagonals_size
    assert size(1440, 11, 11) == 2 * 23 * 1472 * 4                   # Df and Db, [W][roundup(S, 64)] fp32
    assert size(64, 1, 2) == 2 * 4 * 64 * 4 and size(65, 1, 2) == 2 * 4 * 128 * 4 and size(1, 0, 0) == 2 * 64 * 4
    assert size(37, 36, 36) == 2 * 73 * 64 * 4 == size(37, 500, 36)   # (the reaches clamped to S - 1)
    assert size(4096, 31, 32) == 2 * 64 * 4096 * 4
    for bad in [(0, 1, 1), (-4, 1, 1), (64, -1, 1), (64, 1, -1)]:
        assert size(*bad) == 0


# ---- 3. every argument code ------------------------------------------------------------------------------------------------

def test_the_entries_check_every_argument_before_any_device_work():
    lib = _lib.load()
    B, S, cap, out_cap, Tc = 2, 8, 16, 4, 3
    need = lib.torbi_hip_stream_posterior_state_size(B, S, cap)
    p = ctypes.c_void_p(4096)                                 # never dereferenced: every case below fails its checks

    def prepare(trans=p, S=S, left=1, right=2, background=-3., diag=p, ok=p):
        return lib.torbi_hip_stream_smooth_band_prepare(trans, S, left, right, background, diag, ok, 0, None)

    def push(obs=p, Tc=Tc, info=p, diag=p, left=1, right=2, background=-3., initial=p, state=p, nbytes=need, cap=cap, out=p,
             out_cap=out_cap, counts=None, lag=2, B=B, S=S):
        return lib.torbi_hip_stream_smooth_band_push(obs, Tc, info, diag, left, right, background, initial, state, nbytes, cap, out,
                                                     out_cap, counts, lag, B, S, 0, None)

    def flush(info=p, diag=p, left=1, right=2, background=-3., state=p, nbytes=need, cap=cap, out=p, out_cap=out_cap, counts=None,
              B=B, S=S):
        return lib.torbi_hip_stream_smooth_band_flush(info, diag, left, right, background, state, nbytes, cap, out, out_cap, counts, B,
                                                      S, 0, None)

    for bad in [dict(trans=None), dict(diag=None), dict(ok=None), dict(S=0), dict(S=-2), dict(left=-1), dict(right=-1)]:
        assert prepare(**bad) == EINVAL, bad
    for bad in [dict(S=MAX_STATES + 1), dict(S=1440, left=32, right=32), dict(background=math.nan), dict(background=math.inf)]:
        assert prepare(**bad) == EUNSUPPORTED, bad

    for bad in [dict(obs=None), dict(info=None), dict(diag=None), dict(initial=None), dict(state=None), dict(out=None), dict(B=0),
                dict(S=0), dict(B=-3), dict(cap=0), dict(out_cap=0), dict(lag=-1), dict(Tc=-1), dict(left=-1), dict(right=-1)]:
        assert push(**bad) == EINVAL, bad
    for bad in [dict(info=None), dict(diag=None), dict(state=None), dict(out=None), dict(B=0), dict(S=-1), dict(cap=0),
                dict(out_cap=0), dict(left=-1), dict(right=-1)]:
        assert flush(**bad) == EINVAL, bad
    # the dense entries' bound on S stands in front of the band's own
    big = lib.torbi_hip_stream_posterior_state_size(B, 8001, cap)
    assert push(S=8001, nbytes=big) == ERANGE and flush(S=8001, nbytes=big) == ERANGE
    assert push(nbytes=need - 1) == EWORKSPACE and flush(nbytes=need - 1) == EWORKSPACE
    assert push(nbytes=0) == EWORKSPACE and push(cap=cap + 1) == EWORKSPACE
    # what _covers turns down: one state too many, one diagonal too many, a background that is no value of a log matrix
    over = lib.torbi_hip_stream_posterior_state_size(B, MAX_STATES + 1, cap)
    wide = lib.torbi_hip_stream_posterior_state_size(B, 1440, cap)
    for call in (push, flush):
        assert call(S=MAX_STATES + 1, nbytes=over) == EUNSUPPORTED
        assert call(S=1440, left=32, right=32, nbytes=wide) == EUNSUPPORTED
        assert call(background=math.nan) == EUNSUPPORTED and call(background=math.inf) == EUNSUPPORTED


# ---- 4. the constructor and the route query ----------------------------------------------------------------------------

def test_the_route_defaults_to_dense_and_a_bogus_one_is_turned_down():
    import inspect
    parameters = inspect.signature(torbi_amd.StreamPosteriors.__init__).parameters
    assert parameters['route'].default == 'dense' and parameters['band'].default is None
    for route in ('sparse', '', None, 3, 'Dense'):
        with pytest.raises(ValueError):
            torbi_amd.StreamPosteriors(1, 3, gpu=None, route=route)
        with pytest.raises(ValueError):
            torbi_amd.StreamPosteriors(1, 3, gpu=0, route=route)      # (turned down before anything touches a device)


def test_a_band_with_the_dense_route_a_negative_reach_and_a_malformed_tuple_are_turned_down():
    for gpu in (None, 0):                                             # (turned down before anything touches a device)
        with pytest.raises(ValueError):
            torbi_amd.StreamPosteriors(1, 8, gpu=gpu, band=(1, 2, -3.))                    # route='dense' is the default
        with pytest.raises(ValueError):
            torbi_amd.StreamPosteriors(1, 8, gpu=gpu, route='dense', band=(1, 2, -3.))
        for band in [(-1, 2, -3.), (1, -2, -3.), (1, 2), (1, 2, -3., 0), 5, 'abc', (1.5, 2, -3.), (1, 2, 'x'), (1, None, -3.)]:
            for route in ('band', 'auto'):
                with pytest.raises(ValueError):
                    torbi_amd.StreamPosteriors(1, 8, gpu=gpu, route=route, band=band)


@pytest.mark.parametrize('log_probs', [True, False])
def test_without_a_device_every_route_is_the_host_route_and_gives_its_rows(log_probs):
    B, S, T, lag = 2, 9, 12, 2
    obs, trans, init, band = band_problem(B, T, S, 2, 1, BACKGROUNDS[1 + log_probs], log_probs, seed=4)
    runs = []
    for kw in (dict(), dict(route='dense'), dict(route='auto'), dict(route='band'), dict(route='band', band=band),
               dict(route='auto', band=band), dict(route='band', band=(0, 0, 0.))):    # (a band that is not the matrix's: ignored)
        sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=log_probs, gpu=None, lag=lag, **kw)
        assert sp.route == 'host'
        fd = Feeder(sp, obs, trans, init, log_probs, HOST_GAMMA)
        got = []
        for Tc, f in [(5, [5, 2]), (1, [0, 1]), (6, [6, 6])]:
            got += [bits(r) for r in fd.push(Tc, f)] + [bits(sp.filtered()), bits(sp.log_likelihood)]
        rest, final = fd.flush()
        runs.append(got + [bits(r) for r in rest] + [bits(final)])
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(np.array_equal(x, y) for x, y in zip(runs[0], other))


def test_the_route_query_answers_host_without_a_device_and_dense_without_a_matrix():
    assert torbi_amd.stream_posterior_route(None, 2, 64, gpu=None) == 'host'
    _, trans, _, _ = band_problem(1, 1, 64, 1, 2, -math.inf, True, seed=1)
    assert torbi_amd.stream_posterior_route(trans, 2, 64, gpu=None, log_probs=True) == 'host'
    assert torbi_amd.stream_posterior_route(None, 2, 64, gpu=0) == 'dense'     # (answered before anything touches a device)
