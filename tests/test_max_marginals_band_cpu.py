"""The band route of max-marginals without a device: the numpy restatement of the band rule
(tests/max_marginal_band_cases.py) against the full-row loop of the contract (`max_marginal_cases.loop`), by value with equal
NaN positions; the C ABI of torbi_hip_max_marginals_band* as far as it answers before a device is touched; the `route=`
argument of `margins.max_marginals`."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, band_route, inputs, margins, viterbi

import max_marginal_band_cases as mbc
import max_marginal_cases as mmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['torbi_hip_max_marginals_band_covers', 'torbi_hip_max_marginals_band_workspace_size', 'torbi_hip_max_marginals_band']


# ------------------------------------------------------------------------------------------------------- 1: the rule
@pytest.mark.parametrize('background', list(mbc.BACKGROUNDS))
@pytest.mark.parametrize('S,left,right', mbc.REACH_CASES + [(68, 3, 2), (132, 31, 31), (132, 0, 3)],
                         ids=lambda v: str(v))
def test_the_band_rule_equals_the_full_row_loop(S, left, right, background):
    obs, frames, A, pi, want = mbc.case(3, 6, S, left, right, background, seed=S + left)
    assert frames[0] == 6 and frames[-1] == 1
    got = mbc.restate(obs, frames, A, pi, left, right, mbc.BACKGROUNDS[background])
    mmc.same(got, want, (S, left, right, background))
    j = np.arange(S)
    whole = int(((j - left <= 0) & (j + right >= S - 1)).sum())      # rows whose band is the whole row: -inf from the second term
    if (left, right) == (40, 20):
        assert whole == 0 and int((j - left <= 0).sum()) == 41 and int((j + right >= S - 1).sum()) == 21
    if (left, right) == (40, 30):
        assert whole == 8


def test_grid_inputs_are_path_consistent():
    """Every sum exact: max_j m_t[j] == score at every frame, with a grid background inside the in-band range."""
    obs, frames, A, pi, want = mbc.case(3, 6, 64, 3, 2, -1.0, seed=5, grid=4)
    got = mbc.restate(obs, frames, A, pi, 3, 2, -1.0)
    mmc.same(got, want)
    mmc.check_path_consistency(got, frames)


def test_one_case_lets_each_term_decide_a_quarter_of_the_cells():
    """A condition on the inputs, not a measurement: in BOTH_TERMS the out-of-band term strictly decides at least 25 % of
    the cells of each pass and the in-band term at least 25 %; with log(tiny) outside the band it decides next to none, so
    that background alone would never exercise the scans."""
    B, T, S, left, right, background = mbc.BOTH_TERMS
    obs, frames, A, pi, want = mbc.case(*mbc.BOTH_TERMS)
    m, score, decided = mbc.restate(obs, frames, A, pi, left, right, mbc.BACKGROUNDS[background])
    mmc.same((m, score), want)
    for which, (out, inside) in mbc.decided_shares(decided).items():
        assert out >= .25 and inside >= .25, (which, out, inside)
    assert decided['forward'][2] == decided['backward'][2] == S * sum(int(f) - 1 for f in mmc.clamp(frames, T))
    obs, frames, A, pi, _ = mbc.case(B, T, S, left, right, 'log_tiny')
    quiet = mbc.decided_shares(mbc.restate(obs, frames, A, pi, left, right, mbc.BACKGROUNDS['log_tiny'])[2])
    assert all(out < .01 for out, _ in quiet.values())


@pytest.mark.parametrize('value', [math.nan, math.inf])
def test_restatement_follows_the_non_finite_rule_and_the_promise(value):
    obs, frames, A, pi, _ = mbc.case(3, 6, 64, 3, 2, 'log_tiny')
    dirty = np.array(A)
    dirty[5, 4] = value                                              # inside the band
    mmc.same(mbc.restate(obs, frames, dirty, pi, 3, 2, mbc.BACKGROUNDS['log_tiny']), mmc.loop(obs, frames, dirty, pi))
    stray = np.array(A)
    stray[5, 40] = np.float32(-1.)                                   # outside the band: the promise is broken
    m, score, _ = mbc.restate(obs, frames, stray, pi, 3, 2, mbc.BACKGROUNDS['log_tiny'])
    F = mmc.clamp(frames, 6)
    assert np.isnan(score).all() and all(np.isnan(m[b, :F[b]]).all() and (m[b, F[b]:] == mmc.NINF).all() for b in range(3))


# ---------------------------------------------------------------------------------------------------- 2: the C ABI
def test_symbols_are_declared_and_exported_within_abi_17():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r'\b(?:int|size_t) ' + name + r'\s*\(', header), name
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert not name.endswith('_bytes')
    assert _lib.SYMBOLS['torbi_hip_max_marginals_band_workspace_size'][0] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert re.search(r'#define TORBI_HIP_ABI_VERSION 17\b', header)
    for name in ('forward_backward_max_banded', 'max_marginals_banded_workspace_bytes', 'max_marginals_route'):
        assert name in margins.__all__ and callable(getattr(margins, name)) and name not in torbi_amd.__all__
    assert inspect.signature(margins.max_marginals).parameters['route'].default == 'dense'
    assert inspect.signature(margins.forward_backward_max_banded).parameters['background'].default == -math.inf


def test_workspace_size_follows_the_layout():
    lib = _lib.load()
    size = lib.torbi_hip_max_marginals_band_workspace_size
    up = lambda x: -(-x // 256) * 256
    for B, T, S, left, right in [(3, 5, 64, 2, 2), (512, 500, 1440, 11, 11), (512, 500, 1440, 87, 87), (7, 1, 256, 0, 3),
                                 (1, 3, 3072, 253, 254)]:      # (monotone up to the window of 508)
        need = size(B, T, S, left, right)
        assert need == up(4 * (left + right + 1) * S) + up(4 * (B + 1)) + 256 + 256        # diagonals, alarms, verdict, base
        assert need % 256 == 0 and margins.max_marginals_banded_workspace_bytes(B, T, S, left, right) == need
        assert size(B, T + 7, S, left, right) == need                                      # no region grows with T
        assert size(B + 64, T, S, left, right) >= need and size(B, T, S, left + 1, right) >= need
        assert size(B, T, S + 4, left, right) >= need
    # no (B, T, S) region and no beta rows: far below the dense route's
    assert size(512, 500, 1440, 11, 11) < lib.torbi_hip_max_marginals_workspace_size(512, 500, 1440, 0) // 50
    for nonsense in [(0, 5, 64, 2, 2), (3, 0, 64, 2, 2), (3, 5, 0, 2, 2), (3, 5, 64, -1, 2), (3, 5, 64, 2, -1),
                     (3, 5, 16388, 2, 2), (3, 5, 1440, 254, 255)]:
        assert size(*nonsense) == 256, nonsense


def test_covers_answers_without_a_device():
    covers = _lib.load().torbi_hip_max_marginals_band_covers
    f = ctypes.c_float
    for bg in (-math.inf, float(mbc.BACKGROUNDS['log_tiny']), -3., 0., 5.):
        assert covers(1, 1, 1440, 11, 11, f(bg), 0) == 1 and covers(512, 500, 1440, 87, 87, f(bg), 0) == 1
    for S, want in [(60, 0), (62, 0), (64, 1), (3072, 1), (3076, 0), (66, 0), (1441, 0)]:
        assert covers(2, 3, S, 2, 2, f(-math.inf), 0) == want, S
    assert covers(1, 2, 1440, 254, 254, f(0.), 0) == 1 and covers(1, 2, 1440, 254, 255, f(0.), 0) == 0     # windows 508, 509
    assert covers(1, 3, 3072, 254, 254, f(0.), 0) == 1 and covers(1, 3, 3072, 508, 0, f(0.), 0) == 1
    assert mbc.lds_bytes(1, 3072, 508, 0) <= mbc.MAX_LDS                                 # the G = 1 tile always fits
    assert covers(1, 2, 1440, 2, 2, f(math.nan), 0) == 0 and covers(1, 2, 1440, 2, 2, f(math.inf), 0) == 0
    assert covers(0, 2, 1440, 2, 2, f(0.), 0) == 0 and covers(1, 0, 1440, 2, 2, f(0.), 0) == 0
    assert covers(1, 2, 1440, -1, 2, f(0.), 0) == 0 and covers(1, 2, 1440, 2, -1, f(0.), 0) == 0
    assert covers(1, 2, 64, 40, 20, f(-3.), 0) == 1                                      # a band wider than the row


def test_band_entry_answers_bad_arguments_before_any_device_work():
    lib = _lib.load()
    EINVAL, EWORKSPACE, ERANGE, EUNSUPPORTED = -1, -2, -3, -5
    p = ctypes.c_void_p(16)                  # never dereferenced: every call below fails its argument check first
    st = ctypes.c_void_p(0)
    B, T, S = 3, 5, 64
    need = lib.torbi_hip_max_marginals_band_workspace_size(B, T, S, 2, 2)

    def call(obs=p, frames=p, trans=p, init=p, left=2, right=2, bg=-math.inf, marginals=p, scores=p, ws=p, nbytes=need, B=B,
             T=T, S=S):
        return lib.torbi_hip_max_marginals_band(obs, frames, trans, init, left, right, ctypes.c_float(bg), marginals, scores, ws,
                                                nbytes, B, T, S, 0, st)

    assert call(nbytes=need - 1) == EWORKSPACE and call(nbytes=0) == EWORKSPACE
    assert call(left=-1) == EINVAL and call(right=-1) == EINVAL
    assert call(T=0) == EINVAL and call(S=0) == EINVAL and call(B=-1) == EINVAL
    for name in ('obs', 'frames', 'trans', 'init', 'marginals', 'scores', 'ws'):
        assert call(**{name: None}) == EINVAL, name
    assert call(S=66) == EUNSUPPORTED and call(S=60) == EUNSUPPORTED and call(S=3076) == EUNSUPPORTED
    assert call(bg=math.nan) == EUNSUPPORTED and call(bg=math.inf) == EUNSUPPORTED
    assert call(left=254, right=255) == EUNSUPPORTED
    assert call(S=16388) == ERANGE and call(B=1 << 20, T=1 << 13) == ERANGE                 # as the dense entry
    assert lib.torbi_hip_max_marginals(p, p, p, p, p, p, p, 1 << 40, 3, 5, 16388, 0, st) == ERANGE
    assert call(obs=None, frames=None, trans=None, init=None, marginals=None, scores=None, ws=None, nbytes=0, B=0) == 0


def test_instance_rule():
    """The G a shape runs, by the rule the header states: what the device tests choose their batch sizes from."""
    assert mbc.items_per_workgroup(512, 1440, 11, 11) == 2 and mbc.items_per_workgroup(1024, 1440, 11, 11) == 4
    assert mbc.items_per_workgroup(1024, 64, 3, 2) == 4 and mbc.items_per_workgroup(1021, 64, 3, 2) == 4
    assert mbc.items_per_workgroup(1020, 64, 3, 2) == 2 and mbc.items_per_workgroup(510, 64, 3, 2) == 1
    assert mbc.items_per_workgroup(9, 64, 3, 2) == 1
    assert mbc.lds_bytes(4, 3072, 254, 254) > mbc.MAX_LDS >= mbc.lds_bytes(2, 3072, 254, 254)


# ------------------------------------------------------------------------------------------------------- 3: routes
def problem(B=2, T=4, S=64):
    g = torch.Generator().manual_seed(1)
    obs = torch.softmax(torch.randn(B, T, S, generator=g), 2)
    A = torch.softmax(torch.randn(S, S, generator=g), 0)
    return obs, A


def test_route_names_are_checked_first():
    obs, A = problem()
    for route in ('banded', '', None, 'Dense'):
        with pytest.raises(RuntimeError, match="route must be 'auto', 'dense' or 'band'"):
            margins.max_marginals(obs, transition=A, gpu=None, route=route)
    m, score = margins.max_marginals(obs, transition=A, gpu=None, route='dense')
    for route in ('auto',):                                          # the host route ignores 'auto'
        again = margins.max_marginals(obs, transition=A, gpu=None, route=route)
        assert torch.equal(again[0], m) and torch.equal(again[1], score)


def test_band_needs_a_device_and_a_matrix():
    obs, A = problem()
    with pytest.raises(RuntimeError, match=r"max_marginals\(route='band'\) needs a HIP device"):
        margins.max_marginals(obs, transition=A, gpu=None, route='band')
    with pytest.raises(RuntimeError, match=r"max_marginals\(route='band'\): there is no transition matrix"):
        margins.max_marginals(obs, transition=None, gpu=0, route='band')
    with pytest.raises(RuntimeError, match='needs a transition matrix and an initial distribution'):
        margins.forward_backward_max_banded(torch.log(obs), None, None, torch.zeros(64), 2, 2)
    with pytest.raises(RuntimeError, match='reach_left and reach_right must be >= 0'):
        margins.forward_backward_max_banded(torch.log(obs), None, torch.log(A), torch.zeros(64), -1, 2)
    with pytest.raises(RuntimeError, match='forward_backward_max_banded does not cover B=2, T=4, S=64, reach 254/255'):
        margins.forward_backward_max_banded(torch.log(obs), None, torch.log(A), torch.zeros(64), 254, 255)
    assert margins.max_marginals_route(None, 2, 4, 64) == 'uniform'
    assert margins.max_marginals_route(A, 2, 4, 64, gpu=None) == 'dense'
    with pytest.raises(RuntimeError, match='transition must have shape'):
        margins.max_marginals_route(A, 2, 4, 68)


@pytest.mark.parametrize('route', band_route.ROUTES)
def test_dense_never_asks_for_a_plan(monkeypatch, route):
    """'dense' neither plans nor looks at the matrix; 'band' takes what the planner answers; 'auto' asks the planner and takes
    the band only in a class of `_AUTO_BAND`."""
    BAND = (1, 2, -20.)
    asked = {'plan': 0, 'look': 0}
    plan = band_route.plan

    def counting_plan(*args, **kwargs):
        asked['plan'] += 1
        return plan(*args, **kwargs)

    def band_over(trans, original, states):
        asked['look'] += 1
        return BAND

    monkeypatch.setattr(band_route, 'plan', counting_plan)
    monkeypatch.setattr(viterbi, 'band_over', band_over)
    monkeypatch.setattr(margins, '_covered', lambda *args: True)
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: torch.device('cpu'))
    monkeypatch.setattr(margins, '_run', lambda *args: 'dense')
    monkeypatch.setattr(margins, '_run_band', lambda obs, frames, trans, init, *band: band)
    obs, A = problem()
    got = margins.max_marginals(obs, transition=A, gpu=0, route=route)
    if route == 'dense':
        assert got == 'dense' and asked == {'plan': 0, 'look': 0}
    elif route == 'band':
        assert got == BAND and asked == {'plan': 1, 'look': 1}
    else:
        pays = margins._band_pays(2, 64, 1, 2)
        assert got == (BAND if pays else 'dense') and asked == {'plan': 1, 'look': 1}
    # the uniform model has no matrix to plan for
    asked.update(plan=0, look=0)
    if route != 'band':
        assert margins.max_marginals(obs, transition=None, gpu=0, route=route) == 'dense' and asked == {'plan': 0, 'look': 0}


def test_band_raises_with_the_planner_s_reason(monkeypatch):
    monkeypatch.setattr(viterbi, 'band_over', lambda *args: None)
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: torch.device('cpu'))
    monkeypatch.setattr(margins, '_run', lambda *args: 'dense')
    obs, A = problem()
    with pytest.raises(RuntimeError) as raised:
        margins.max_marginals(obs, transition=A, gpu=0, route='band')
    assert str(raised.value).startswith("max_marginals(route='band'): the matrix does not hold one value outside a band")
    assert margins.max_marginals(obs, transition=A, gpu=0, route='auto') == 'dense'
    monkeypatch.setattr(viterbi, 'band_over', lambda *args: (1, 2, -20.))
    monkeypatch.setattr(margins, '_covered', lambda *args: False)
    with pytest.raises(RuntimeError) as raised:
        margins.max_marginals(obs, transition=A, gpu=0, route='band')
    assert str(raised.value) == ("max_marginals(route='band'): torbi_hip_max_marginals_band_covers turns down batch=2, frames=4, "
                                 'states=64, reach 1/2, background -20.0')


def test_auto_classes_lie_inside_what_was_measured():
    """`_AUTO_BAND` lists classes of (smallest batch, largest batch, diagonals of 1440 states); the probe measured batches 1, 8
    and 512 and bands of 23 and 175 diagonals, so nothing beyond those may be listed."""
    for low, high, diagonals in margins._AUTO_BAND:
        assert 1 <= low <= high <= 512 and diagonals in (23, 175)
    assert not margins._band_pays(513, 1440, 11, 11) and not margins._band_pays(1, 1440, 88, 88)
