"""torbi_amd.StreamDecoder(max_lag=...) on the host (gpu=None) and torbi_hip_stream_push_lag's argument checks (no device):
the bounded push against the brute-force rule of tests/stream_lag_cases.py after every push."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, synth
from stream_cases import plan
from stream_lag_cases import feed_bounded, identity, reference_prefix_check, nonfinite_scenario, flush_scenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decoder(B, S, trans, init, max_lag):
    return torbi_amd.StreamDecoder(B, S, torch.from_numpy(trans), torch.from_numpy(init), log_probs=True, gpu=None, max_lag=max_lag)


def problem(kind, B, T, S, seed):
    """(source, transition, initial) of one matrix kind; the all-zero case scores everything 0, so every argmax is a tie."""
    obs, trans, init = synth.problem(B, T, S, seed=seed)
    if kind == 'band':
        trans = synth.banded_transition(S, min(3, S))
    elif kind == 'identity':
        trans = identity(S)
    elif kind == 'zero':
        obs, trans, init = np.zeros_like(obs), np.zeros_like(trans), np.zeros_like(init)
    return [obs[b] for b in range(B)], trans, init


def plans(B, T, seed):
    fixed = [(3, np.minimum(3, T - t) * np.ones(B, dtype=np.int64)) for t in range(0, T, 3)]
    return {'one': plan(B, T, 'one'), 'ragged': plan(B, T, 'ragged', seed=seed), 'fixed': fixed}


# ------------------------------------------------------------------------------------------------ 1: the prefix property
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('kind', ['dense', 'band', 'identity', 'zero'])
@pytest.mark.parametrize('S', [1, 2, 3, 5, 63, 65])
def test_every_push_is_a_span_of_the_whole_decode_of_the_frames_so_far(S, kind, B):
    """max_lag 0, 1, 3, 8 x pushes of one frame, ragged pushes and pushes of 3: outputs, `pending == min(natural, max_lag)`
    and `forced` after every push (feed_bounded)."""
    T = 18
    source, trans, init = problem(kind, B, T, S, seed=S + B)
    reference_prefix_check(source[0], trans, init, T // 2)
    for max_lag in (0, 1, 3, 8):
        for name, pushes in plans(B, T, seed=S + max_lag).items():
            dec = decoder(B, S, trans, init, max_lag)
            feed_bounded(dec, source, trans, init, pushes)
            assert dec.capacity <= max_lag + max(Tc for Tc, _ in pushes) + 1, (max_lag, name, dec.capacity)
    if kind == 'identity' and S > 1:                           # nothing is ever decided: every returned frame is forced
        dec = decoder(B, S, trans, init, 3)
        for t in range(T):
            dec.push(torch.from_numpy(np.stack(source)[:, t:t + 1]))
        assert dec.forced.tolist() == [T - 3] * B and dec.pending.tolist() == [3] * B


# ------------------------------------------------------------------------------------------- 2: a lag that never binds
@pytest.mark.parametrize('kind,S', [('dense', 5), ('dense', 65), ('band', 63)])
@pytest.mark.parametrize('mode', ['one', 'ragged'])
def test_a_lag_of_the_largest_natural_pending_changes_nothing(kind, S, mode):
    B, T = 3, 30
    source, trans, init = problem(kind, B, T, S, seed=7 + S)
    pushes = plan(B, T, mode, seed=S)
    most = [0]

    def watch(k, dec):
        most[0] = max(most[0], int(dec.pending.max()))
    exact, _ = feed_bounded(decoder(B, S, trans, init, None), source, trans, init, pushes, after=watch)
    assert most[0] >= 1
    dec = decoder(B, S, trans, init, most[0])
    seen = []
    bounded, _ = feed_bounded(dec, source, trans, init, pushes, after=lambda k, d: seen.append(d.forced.tolist()))
    assert all(row == [0] * B for row in seen)
    for k, (a, o) in enumerate(zip(exact, bounded)):
        assert all(np.array_equal(x, y) for x, y in zip(a, o)), k
    # one frame less, and the bound binds: the comparison above is not vacuous
    tight = decoder(B, S, trans, init, most[0] - 1)
    seen = []
    feed_bounded(tight, source, trans, init, pushes, after=lambda k, d: seen.append(int(d.forced.sum())))
    assert max(seen) >= 1


# ------------------------------------------------------------------------------------------------------ 3: NaN and -inf
@pytest.mark.parametrize('max_lag', [0, 2])
def test_forced_path_starts_at_the_first_nan_and_ties_of_minus_infinity_go_to_state_0(max_lag):
    nonfinite_scenario(decoder, max_lag)


# --------------------------------------------------------------------------------------------------- 4: flush half-way
def test_flush_of_one_stream_half_way_restarts_it_and_leaves_its_neighbours():
    flush_scenario(decoder)


# -------------------------------------------------------------------------------------------------------- 5: arguments
@pytest.mark.parametrize('bad', [-1, 1.5, 'x'])
def test_max_lag_must_be_none_or_a_non_negative_integer(bad):
    with pytest.raises(ValueError):
        torbi_amd.StreamDecoder(2, 3, gpu=None, max_lag=bad)


def test_max_lag_none_zero_and_numpy_integers_are_accepted():
    assert torbi_amd.StreamDecoder(2, 3, gpu=None).max_lag is None
    assert torbi_amd.StreamDecoder(2, 3, gpu=None, max_lag=0).max_lag == 0
    assert torbi_amd.StreamDecoder(2, 3, gpu=None, max_lag=np.int64(4)).max_lag == 4
    dec = torbi_amd.StreamDecoder(2, 3, gpu=None, max_lag=4)
    assert dec.forced.tolist() == [0, 0] and dec.forced.dtype == torch.int64 and dec.capacity == 0


# ------------------------------------------------------------------------------------------------------------ 6: C ABI
def test_push_lag_answers_bad_arguments_as_the_push_does():
    """Every argument set tests/test_host_cpu.py's stream test gives torbi_hip_stream_push: push_lag(..., -1, NULL, ...)
    returns the same code; then the entry's own two EINVAL cases, which come after the push's arguments.  Every call is turned
    down before a device is touched; the pointers are host memory nobody reads."""
    lib = _lib.load()
    EINVAL, EWORKSPACE, ERANGE = -1, -2, -3
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, S, cap, out_cap = 3, 5, 4, 6
    need = lib.torbi_hip_stream_state_bytes(B, S, cap)

    def both(lag=-1, forced=null, obs=p, Tc=2, info=p, trans=p, tt=p, init=p, state=p, nbytes=need, cap=cap, out=p,
             out_cap=out_cap, counts=p, B=B, S=S):
        plain = lib.torbi_hip_stream_push(obs, Tc, info, trans, tt, init, state, nbytes, cap, out, out_cap, counts, B, S, 0, null)
        bounded = lib.torbi_hip_stream_push_lag(obs, Tc, info, trans, tt, init, state, nbytes, cap, out, out_cap, counts, lag,
                                                forced, B, S, 0, null)
        return plain, bounded
    sets = [{name: null} for name in ('info', 'trans', 'state', 'out', 'counts')]
    sets += [{name: value} for name in ('B', 'S', 'cap', 'out_cap') for value in (0, -1)]
    sets += [dict(nbytes=need - 1), dict(nbytes=0), dict(cap=cap + 1), dict(S=8001, nbytes=1 << 40), dict(S=8001),
             dict(S=8001, info=null), dict(S=8001, cap=0), dict(S=8000), dict(Tc=-1), dict(Tc=-1, nbytes=0)]
    for name in ('obs', 'tt', 'init'):
        sets += [{name: null}, {name: null, 'nbytes': 0}, {name: null, 'S': 8001}]
    seen = set()
    for kwargs in sets:
        plain, bounded = both(**kwargs)
        assert plain == bounded and plain in (EINVAL, EWORKSPACE, ERANGE), (kwargs, plain, bounded)
        seen.add(plain)
        # a lag with its array changes none of these answers either
        assert both(lag=3, forced=p, **kwargs)[1] == plain, kwargs
    assert seen == {EINVAL, EWORKSPACE, ERANGE}
    # the entry's own arguments: looked at last
    assert both(lag=-2)[1] == EINVAL and both(lag=-2, forced=p)[1] == EINVAL
    assert both(lag=0)[1] == EINVAL and both(lag=7)[1] == EINVAL                 # a bound without forced_out
    assert both(lag=-2, nbytes=0)[1] == EWORKSPACE and both(lag=0, S=8001)[1] == ERANGE


def test_header_and_symbol_table_declare_push_lag():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    assert re.search(r'\bint torbi_hip_stream_push_lag\s*\(', header)
    declaration = re.search(r'int torbi_hip_stream_push_lag\s*\(([^;]*)\);', header).group(1)
    assert re.search(r'int32_t \*counts_out, int max_lag, int32_t \*forced_out,\s*int B, int S, int device, void \*stream', declaration)
    assert 'torbi_hip_stream_push_lag' in _lib.SYMBOLS
    push, lag = _lib.SYMBOLS['torbi_hip_stream_push'], _lib.SYMBOLS['torbi_hip_stream_push_lag']
    assert lag[0] is ctypes.c_int and lag[1] == push[1][:12] + [ctypes.c_int, ctypes.c_void_p] + push[1][12:]
    assert _lib.load().torbi_hip_stream_push_lag is not None and _lib.ABI_VERSION == 17
