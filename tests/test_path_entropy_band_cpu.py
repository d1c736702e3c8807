"""The band route of path entropy without a device: the float64 numpy restatement of the band split
(tests/path_entropy_band_cases.py) against the full-matrix loop of the contract (`path_entropy_cases.loop`); the weight of
the background terms; the C ABI of torbi_hip_path_entropy_band* as far as it answers before a device is touched; the `route=`
argument of `entropy.path_entropy`."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, band_route, entropy, inputs, viterbi

import path_entropy_band_cases as pbc
import path_entropy_cases as pec
import stream_band_cases as sbc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['torbi_hip_path_entropy_band_covers', 'torbi_hip_path_entropy_band_workspace_size', 'torbi_hip_path_entropy_band']
# the bound the device tests assert on H and the prefix entries (tests/test_path_entropy_band_gpu.py)
RTOL_H, ATOL_H_PER_FRAME = 4e-5, 4e-5


# ------------------------------------------------------------------------------------------------------- 1: the rule
def restated(key):
    obs, frames, A, pi = pbc.case(*key)
    B, T, S, left, right, background = key[:6]
    assert frames[0] == T and (B < 2 or frames[-1] == 1)
    got = pbc.restate(obs, frames, A, pi, left, right, pbc.BACKGROUNDS[background])
    want = pbc.loop_reference(*key)
    for g, w, what in zip(got, want, ('entropy', 'log-likelihood', 'prefix')):
        pec.close(g, w, pec.reference_bound(w), (key, what))
    return got


@pytest.mark.parametrize('background', list(pbc.BACKGROUNDS))
@pytest.mark.parametrize('S,left,right', [(64, left, right) for left, right in sbc.REACHES]
                         + [(5, 10, 10), (5, 4, 9), (65, 2, 5), (70, 3, 0), (200, 2, 5)], ids=lambda v: str(v))
def test_the_band_split_equals_the_full_matrix_loop(S, left, right, background):
    restated((3, 6, S, left, right, background, S + left))


@pytest.mark.parametrize('background', list(pbc.BACKGROUNDS))
def test_the_band_split_with_minus_inf_cells_inside_the_band(background):
    key = (3, 8, 70, 3, 2, background, 11, True)
    A = pbc.case(*key)[2]
    j, i = np.meshgrid(np.arange(70), np.arange(70), indexing='ij')
    inside = (i >= j - 3) & (i <= j + 2)
    assert np.isneginf(A[inside]).any() and np.isfinite(A[inside]).any()
    H, L, prefix = restated(key)
    assert np.isfinite(H).all() and np.isfinite(L).all() and np.isfinite(prefix).all()


def test_the_restatement_answers_a_broken_promise_with_nan():
    key = (3, 6, 64, 2, 5, 'log_tiny', 5)
    obs, frames, A, pi = pbc.case(*key)
    stray = np.array(A)
    stray[40, 3] = np.float32(-1.)
    H, L, prefix = pbc.restate(obs, frames, stray, pi, 2, 5, pbc.BACKGROUNDS['log_tiny'])
    F = pec.clamp(frames, 6)
    assert np.isnan(H).all() and np.isnan(L).all()
    assert all(np.isnan(prefix[b, :F[b]]).all() and (prefix[b, F[b]:] == 0).all() for b in range(3))


def test_the_background_terms_matter():
    """With -3 outside the band, H of the same problem with -inf outside it is further from the true H than 100 times the
    bound of the device tests: a kernel that drops the ebg or the gbg terms cannot pass them."""
    B, T, S, left, right = 2, 64, 1440, 11, 11
    key = (B, T, S, left, right, 'minus_3', 3)
    obs, frames, A, pi = pbc.case(*key)
    true_H = restated(key)[0]
    j, i = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    cut = np.where((i >= j - left) & (i <= j + right), A, np.float32(-np.inf)).astype(np.float32)
    dropped = pbc.restate(obs, frames, cut, pi, left, right, -np.inf)[0]
    bound = RTOL_H * abs(true_H[0]) + ATOL_H_PER_FRAME * T
    print(f'H with -3 outside the band {true_H[0]:.2f}, with -inf outside it {dropped[0]:.2f}, bound {bound:.2e}')
    assert abs(true_H[0] - dropped[0]) > 100 * bound
    assert 150 < true_H[0] - dropped[0] < 200 and 200 < true_H[0] < 250              # (about 226 against 51 nats)


# ---------------------------------------------------------------------------------------------------- 2: the C ABI
def test_symbols_are_declared_and_exported_within_abi_17():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r'\b(?:int|size_t) ' + name + r'\s*\(', header), name
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert not name.endswith('_bytes')
    assert _lib.SYMBOLS['torbi_hip_path_entropy_band_workspace_size'][0] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 17 and lib.torbi_hip_abi_version() == 17
    assert re.search(r'#define TORBI_HIP_ABI_VERSION 17\b', header)
    for name in ('forward_entropy_banded', 'path_entropy_banded_workspace_bytes', 'path_entropy_route'):
        assert name in entropy.__all__ and callable(getattr(entropy, name)) and name not in torbi_amd.__all__
    assert inspect.signature(entropy.path_entropy).parameters['route'].default == 'dense'
    banded = inspect.signature(entropy.forward_entropy_banded).parameters
    assert banded['background'].default == -math.inf and banded['prefix'].default is False
    assert list(banded) == ['observation', 'batch_frames', 'transition', 'initial', 'reach_left', 'reach_right', 'background',
                            'workspace', 'prefix']


def test_covers_truth_table():
    covers = _lib.load().torbi_hip_path_entropy_band_covers
    f = ctypes.c_float
    for bg in (-math.inf, float(sbc.TINY), -3., 0., 5.):
        assert covers(1, 1, 1440, 11, 11, f(bg), 0) == 1 and covers(512, 500, 1440, 11, 11, f(bg), 0) == 1
    assert covers(512, 500, 1440, 87, 87, f(-math.inf), 0) == 0                       # 175 diagonals: beyond the window
    for S, want in [(1, 1), (3, 1), (65, 1), (1441, 1), (4096, 1), (4097, 0), (0, 0)]:
        assert covers(2, 3, S, 2, 2, f(-math.inf), 0) == want, S
    assert covers(1, 2, 1440, 31, 32, f(0.), 0) == 1 and covers(1, 2, 1440, 32, 32, f(0.), 0) == 0       # windows 64, 65
    assert covers(1, 2, 1440, 63, 0, f(0.), 0) == 1 and covers(1, 2, 1440, 0, 64, f(0.), 0) == 0
    assert covers(1, 2, 64, 200, 200, f(-3.), 0) == 1 and covers(1, 2, 65, 200, 200, f(-3.), 0) == 0     # clamped to S - 1
    assert covers(1, 2, 1440, 2, 2, f(math.nan), 0) == 0 and covers(1, 2, 1440, 2, 2, f(math.inf), 0) == 0
    assert covers(0, 2, 1440, 2, 2, f(0.), 0) == 0 and covers(1, 0, 1440, 2, 2, f(0.), 0) == 0
    assert covers(1, 2, 1440, -1, 2, f(0.), 0) == 0 and covers(1, 2, 1440, 2, -1, f(0.), 0) == 0
    # torbi_hip_path_entropy's limits on B and T
    assert covers(1 << 20, 1 << 13, 64, 2, 2, f(0.), 0) == 0 and covers(32 * 65535 + 1, 1, 64, 2, 2, f(0.), 0) == 0
    assert covers(32 * 65535, 1, 64, 2, 2, f(0.), 0) == 1
    # the LDS edge: one item's rows must fit the budget; the largest rows the window admits (4096 states, a halo of 63) do,
    # so within the other limits the budget refuses nothing -- and four such items no longer fit
    assert covers(1, 2, 4096, 63, 0, f(0.), 0) == 1 and covers(1, 2, 4096, 0, 63, f(0.), 0) == 1
    assert pbc.lds_bytes(1, 4096, 63, 0) <= pbc.MAX_LDS < pbc.lds_bytes(4, 4096, 63, 0)
    assert pbc.lds_bytes(1, 4096, 63, 0) == 16 * (4096 + 126) + 524 + 16


def test_workspace_size_follows_the_layout():
    lib = _lib.load()
    size = lib.torbi_hip_path_entropy_band_workspace_size
    up = lambda x: -(-x // 256) * 256
    for B, T, S, left, right in [(3, 5, 64, 2, 2), (512, 500, 1440, 11, 11), (7, 1, 65, 0, 3), (1, 3, 4096, 31, 32),
                                 (2, 9, 5, 10, 10)]:
        W = pbc.clamp_reach(left, S) + pbc.clamp_reach(right, S) + 1
        diagonals = up(4 * W * (-(-S // 64) * 64))
        need = size(B, T, S, left, right)
        # the two sets of diagonals; m, c and the prefix; the flag; room to align the base
        assert need == 2 * diagonals + 3 * up(4 * B * T) + 256 + 256, (B, T, S, left, right)
        assert need % 256 == 0 and entropy.path_entropy_banded_workspace_bytes(B, T, S, left, right) == need
    # no term in B T S: the states enter through the diagonals alone
    assert size(512, 500, 1440, 11, 11) - size(512, 500, 64, 11, 11) == 2 * (up(4 * 23 * 1472) - up(4 * 23 * 64))
    assert size(512, 500, 1440, 11, 11) < lib.torbi_hip_path_entropy_workspace_size(512, 500, 1440, 0) // 9
    for nonsense in [(0, 5, 64, 2, 2), (3, 0, 64, 2, 2), (3, 5, 0, 2, 2), (3, 5, 64, -1, 2), (3, 5, 64, 2, -1), (3, 5, 4097, 2, 2)]:
        assert size(*nonsense) == 256, nonsense


def test_band_entry_answers_bad_arguments_before_any_device_work():
    lib = _lib.load()
    EINVAL, EWORKSPACE, ERANGE, EUNSUPPORTED = -1, -2, -3, -5
    p = ctypes.c_void_p(16)                  # never dereferenced: every call below fails its argument check first
    st = ctypes.c_void_p(0)
    B, T, S = 3, 5, 64
    need = lib.torbi_hip_path_entropy_band_workspace_size(B, T, S, 2, 2)

    def call(obs=p, frames=p, trans=p, init=p, left=2, right=2, bg=-math.inf, H=p, prefix=p, L=p, ws=p, nbytes=need, B=B, T=T,
             S=S):
        return lib.torbi_hip_path_entropy_band(obs, frames, trans, init, left, right, ctypes.c_float(bg), H, prefix, L, ws, nbytes,
                                               B, T, S, 0, st)

    assert call(nbytes=need - 1) == EWORKSPACE and call(nbytes=0) == EWORKSPACE
    assert call(prefix=None, nbytes=need - 1) == EWORKSPACE                              # (a null prefix is no error)
    assert call(left=-1) == EINVAL and call(right=-1) == EINVAL
    assert call(T=0) == EINVAL and call(S=0) == EINVAL and call(B=-1) == EINVAL
    for name in ('obs', 'frames', 'trans', 'init', 'H', 'L', 'ws'):
        assert call(**{name: None}) == EINVAL, name
    assert call(S=4097) == EUNSUPPORTED and call(S=130, left=32, right=32) == EUNSUPPORTED
    assert call(bg=math.nan) == EUNSUPPORTED and call(bg=math.inf) == EUNSUPPORTED
    assert call(S=16388) == ERANGE and call(B=1 << 20, T=1 << 13) == ERANGE              # as the dense entry
    assert lib.torbi_hip_path_entropy(p, p, p, p, p, p, p, p, 1 << 40, 3, 5, 16388, 0, st) == ERANGE
    # the order: an argument error before the range, the range before the cover, the cover before the workspace
    assert call(obs=None, S=16388, nbytes=0) == EINVAL and call(S=16388, bg=math.nan, nbytes=0) == ERANGE
    assert call(bg=math.nan, nbytes=0) == EUNSUPPORTED
    assert call(obs=None, frames=None, trans=None, init=None, H=None, prefix=None, L=None, ws=None, nbytes=0, B=0) == 0


def test_instance_rule():
    """The G a shape runs, by the rule the header states: what the device tests choose their batch sizes from."""
    rule = lambda B, S, left, right: pbc.items_per_workgroup(B, S, left, right, compute_units=256)
    assert rule(512, 1440, 11, 11) == 2 and rule(1024, 1440, 11, 11) == 4 and rule(4096, 1440, 11, 11) == 4
    assert pbc.lds_bytes(8, 1440, 11, 11) > pbc.MAX_LDS >= pbc.lds_bytes(4, 1440, 11, 11)
    assert rule(2048, 64, 3, 2) == 4 and rule(1021, 64, 3, 2) == 4 and rule(1020, 64, 3, 2) == 2
    assert rule(511, 64, 3, 2) == 2 and rule(510, 64, 3, 2) == 1 and rule(9, 64, 3, 2) == 1


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
            entropy.path_entropy(obs, transition=A, gpu=None, route=route)
    want = entropy.path_entropy(obs, transition=A, gpu=None, route='dense', prefix=True)
    again = entropy.path_entropy(obs, transition=A, gpu=None, route='auto', prefix=True)     # the host route ignores 'auto'
    assert all(torch.equal(a, b) for a, b in zip(again, want))
    assert all(torch.equal(a, b) for a, b in zip(entropy.path_entropy(obs, transition=A, gpu=None, prefix=True), want))


def test_band_needs_a_device_and_a_matrix():
    obs, A = problem()
    with pytest.raises(RuntimeError, match=r"path_entropy\(route='band'\) needs a HIP device"):
        entropy.path_entropy(obs, transition=A, gpu=None, route='band')
    with pytest.raises(RuntimeError, match=r"path_entropy\(route='band'\): there is no transition matrix"):
        entropy.path_entropy(obs, transition=None, gpu=0, route='band')
    with pytest.raises(RuntimeError, match='needs a transition matrix and an initial distribution'):
        entropy.forward_entropy_banded(torch.log(obs), None, None, torch.zeros(64), 2, 2)
    with pytest.raises(RuntimeError, match='reach_left and reach_right must be >= 0'):
        entropy.forward_entropy_banded(torch.log(obs), None, torch.log(A), torch.zeros(64), -1, 2)
    with pytest.raises(RuntimeError, match='forward_entropy_banded does not cover B=2, T=4, S=64, reach 2/2, background nan'):
        entropy.forward_entropy_banded(torch.log(obs), None, torch.log(A), torch.zeros(64), 2, 2, math.nan)
    obs, A = problem(S=130)
    with pytest.raises(RuntimeError, match='forward_entropy_banded does not cover B=2, T=4, S=130, reach 32/32'):
        entropy.forward_entropy_banded(torch.log(obs), None, torch.log(A), torch.zeros(130), 32, 32)
    assert entropy.path_entropy_route(None, 2, 4, 64) == 'uniform'
    assert entropy.path_entropy_route(A, 2, 4, 130, gpu=None) == 'dense'
    with pytest.raises(RuntimeError, match='transition must have shape'):
        entropy.path_entropy_route(A, 2, 4, 68)


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
    monkeypatch.setattr(entropy, '_covered', lambda *args: True)
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: torch.device('cpu'))
    monkeypatch.setattr(entropy, '_run', lambda *args: 'dense')
    monkeypatch.setattr(entropy, '_run_band', lambda obs, frames, trans, init, *rest: tuple(rest[:3]))
    obs, A = problem()
    got = entropy.path_entropy(obs, transition=A, gpu=0, route=route)
    if route == 'dense':
        assert got == 'dense' and asked == {'plan': 0, 'look': 0}
    elif route == 'band':
        assert got == BAND and asked == {'plan': 1, 'look': 1}
    else:
        pays = entropy._band_pays(2, 64, 1, 2)
        assert got == (BAND if pays else 'dense') and asked == {'plan': 1, 'look': 1}
        assert entropy.path_entropy_route(A, 2, 4, 64, gpu=0) == ('band' if pays else 'dense')
    # the default is 'dense'
    asked.update(plan=0, look=0)
    assert entropy.path_entropy(obs, transition=A, gpu=0) == 'dense' and asked == {'plan': 0, 'look': 0}
    # the uniform model has no matrix to plan for
    if route != 'band':
        assert entropy.path_entropy(obs, transition=None, gpu=0, route=route) == 'dense' and asked == {'plan': 0, 'look': 0}


def test_band_raises_with_the_planner_s_reason(monkeypatch):
    monkeypatch.setattr(viterbi, 'band_over', lambda *args: None)
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: torch.device('cpu'))
    monkeypatch.setattr(entropy, '_run', lambda *args: 'dense')
    obs, A = problem()
    with pytest.raises(RuntimeError) as raised:
        entropy.path_entropy(obs, transition=A, gpu=0, route='band')
    assert str(raised.value).startswith("path_entropy(route='band'): the matrix does not hold one value outside a band")
    assert entropy.path_entropy(obs, transition=A, gpu=0, route='auto') == 'dense'
    assert entropy.path_entropy_route(A, 2, 4, 64, gpu=0) == 'dense'
    monkeypatch.setattr(viterbi, 'band_over', lambda *args: (1, 2, -20.))
    monkeypatch.setattr(entropy, '_covered', lambda *args: False)
    with pytest.raises(RuntimeError) as raised:
        entropy.path_entropy(obs, transition=A, gpu=0, route='band')
    assert str(raised.value) == ("path_entropy(route='band'): torbi_hip_path_entropy_band_covers turns down batch=2, frames=4, "
                                 'states=64, reach 1/2, background -20.0')


def test_auto_classes_lie_inside_what_was_measured():
    """`_AUTO_BAND` lists classes of (smallest batch, largest batch, diagonals of 1440 states); the probe measured batches 1, 8
    and 512 on 23 diagonals (175 diagonals lie beyond the window of the kernel), so nothing beyond those may be listed."""
    for low, high, diagonals in entropy._AUTO_BAND:
        assert 1 <= low <= high <= 512 and diagonals == 23
    assert not entropy._band_pays(513, 1440, 11, 11) and not entropy._band_pays(1, 1440, 12, 11)
    assert not entropy._band_pays(1, 1440, 87, 87)
