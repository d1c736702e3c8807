"""The band planner (torbi_amd/band_route.py) without a device: `plan` and `choose` as a table over the route, what the
matrix and the feature's covers function answer and whether a look is allowed; then the same table through the few lines each
of the five features keeps, with `viterbi.band_over` and the feature's covers function substituted."""
import itertools
import types

import pytest
import torch

import torbi_amd
from torbi_amd import band_route, k_best, posterior, sampling, state, stream, training, viterbi

B, T, S = 2, 5, 64
BAND = (1, 2, -20.)
NO_BAND = ('the matrix does not hold one value outside a band that viterbi.band_over can answer for (states % 4 == 0, '
           '64 <= states <= 3072, reach_left + reach_right + 4 <= 512, a background that is -inf or {})')
UNKNOWN = 'the structure of the matrix is not known yet'
MATRIX = ('none', 'uncovered', 'covered', 'pays')          # no band; a band not covered; covered, does not pay; covered and pays
LOOKS = ('look', 'known', 'unknown')                        # look=True; look=False on a structure known / not known


class Fakes:
    """`viterbi.band_over` and a covers function that answer what `matrix` says, and count how often they are asked."""

    def __init__(self, monkeypatch, matrix):
        self.matrix, self.looks, self.asked = matrix, 0, []
        monkeypatch.setattr(viterbi, 'band_over', self.band_over)

    def band_over(self, trans, original, states):
        self.looks += 1
        return None if self.matrix == 'none' else BAND

    def covers(self, *args):
        self.asked.append(args)
        return self.matrix in ('covered', 'pays')

    def pays(self, *band):
        assert band == BAND
        return self.matrix == 'pays'


def matrix_for(look):
    """A host matrix whose structure is, or is not, in the notes `plan(look=False)` peeks at."""
    A = torch.zeros((S, S))
    if look == 'known':
        state.notes(A)[('band_over', S)] = BAND
    return A


def expected(route, matrix, look):
    """(band, reason of the plan, whether band_over is asked)."""
    if look == 'unknown':
        return None, UNKNOWN, False
    if matrix == 'none':
        return None, NO_BAND.format('finite'), True
    if matrix == 'uncovered':
        return None, f'some_covers turns down batch={B}, states={S}, reach 1/2, background -20.0', True
    return BAND, '', True


@pytest.mark.parametrize('route,matrix,look', list(itertools.product(band_route.ROUTES, MATRIX, LOOKS)))
def test_plan_and_choose(monkeypatch, route, matrix, look):
    fakes = Fakes(monkeypatch, matrix)
    A = matrix_for(look)
    band, why, looked = expected(route, matrix, look)
    args = (A, A, fakes.covers, 'some_covers', dict(batch=B, states=S), 3)
    assert band_route.plan(*args, look=look == 'look') == (band, why)
    assert fakes.looks == int(looked) and fakes.asked == ([(B, S, *BAND, 3)] if looked and matrix != 'none' else [])
    fakes.looks = 0
    if route == 'band' and band is None:
        with pytest.raises(RuntimeError) as raised:
            band_route.choose(route, band, why, fakes.pays, 'who')
        assert str(raised.value) == f'who: {why}'
    else:
        takes = band if route == 'band' or (route == 'auto' and matrix == 'pays') else None
        assert band_route.choose(route, band, why, fakes.pays, 'who') == takes
        assert band_route.choose(route, band, why, None, 'who') == (None if route == 'dense' else band)
    assert fakes.looks == 0                                                   # `choose` asks nobody


def test_plan_of_an_empty_batch_and_the_other_background_text(monkeypatch):
    fakes = Fakes(monkeypatch, 'none')
    A = torch.zeros((S, S))
    assert band_route.plan(A, A, fakes.covers, 'x', dict(batch=0, states=S)) == (None, 'the batch is empty') and fakes.looks == 0
    finite = 'a finite value below every entry of the band'
    want = NO_BAND.format(finite)
    assert band_route.plan(A, A, fakes.covers, 'x', dict(batch=1, states=S), finite=finite) == (None, want)
    assert stream._band_plan(A, A, 1, S, 0) == (None, want)


def test_route_names_and_stated_bands():
    for error in (RuntimeError, ValueError):
        with pytest.raises(error, match="route must be 'auto', 'dense' or 'band'; got 'banded'") as raised:
            band_route.check_route('banded', error)
        assert type(raised.value) is error
    assert [band_route.check_route(r) for r in band_route.ROUTES] == ['auto', 'dense', 'band']
    assert band_route.stated(2.0, True, 3) == (2, 1, 3.0) and type(band_route.stated(0, 0, -20)[2]) is float
    for reaches in ((-1, 0), (0, -1)):
        with pytest.raises(RuntimeError, match=f'reach_left and reach_right must be >= 0; got {reaches[0]}, {reaches[1]}'):
            band_route.stated(*reaches, 0.)


def test_every_feature_checks_the_route_name_with_its_own_exception():
    obs, A, pi = torch.zeros((B, T, 4)), torch.zeros((4, 4)), torch.zeros(4)
    model = dict(transition=A, initial=pi, log_probs=True, gpu=None, route='banded')
    calls = [(RuntimeError, lambda: torbi_amd.state_posteriors(obs, **model)),
             (RuntimeError, lambda: torbi_amd.expected_counts(obs, **model)),
             (RuntimeError, lambda: torbi_amd.log_likelihood(obs, None, A, pi, route='banded')),
             (RuntimeError, lambda: torbi_amd.sample_paths(obs, **model)),
             (ValueError, lambda: torbi_amd.best_paths(obs, 2, **model)),
             (ValueError, lambda: torbi_amd.decode_k_best(obs, None, A, pi, 2, route='banded')),
             (ValueError, lambda: torbi_amd.StreamDecoder(B, 4, A, pi, log_probs=True, gpu=None, route='banded'))]
    for error, call in calls:
        with pytest.raises(error, match='route must be') as raised:
            call()
        assert type(raised.value) is error


def features(monkeypatch, fakes):
    """name -> (who, the reason's text before the band, route -> band or None): the lines a feature keeps around the planner,
    on host tensors, with the feature's covers function substituted."""
    A, x, f, pi = torch.zeros((S, S)), torch.zeros((B, T, S)), torch.full((B,), T), torch.zeros(S)
    for module, name in ((posterior, '_covered'), (training, '_counts_covered'), (sampling, '_covered'), (k_best, '_covered'),
                         (stream, '_covered')):
        monkeypatch.setattr(module, name, fakes.covers)
    # k-best: `_routed` goes on to the call it chose; the band it hands `_run_band` is the answer
    monkeypatch.setattr(k_best, '_run', lambda *args: None)
    monkeypatch.setattr(k_best, '_run_band', lambda obs, frames, trans, init, k, *rest: rest[:3])
    decoder = types.SimpleNamespace(device=torch.device('cpu'), transition=A, batch=B, states=S)
    return {
        'posteriors': ("state_posteriors(route='band')",
                       f'torbi_hip_forward_backward_band_covers turns down batch={B}, frames={T}, states={S}',
                       lambda route: posterior._band(route, A, A, B, T, S, 0)),
        'sampling': ("sample_paths(route='band')",
                     f'torbi_hip_sample_band_covers turns down batch={B}, frames={T}, states={S}, draws=3',
                     lambda route: sampling._band(route, A, A, B, T, S, 3, 0)),
        'k-best': ("k-best decoding with route='band'",
                   f'torbi_hip_k_best_band_covers turns down batch={B}, frames={T}, states={S}, k=2',
                   lambda route: k_best._routed(x, f, A, A, None, pi, 2, route)),
        'stream': ("StreamDecoder(route='band')", f'torbi_hip_stream_band_covers turns down batch={B}, states={S}',
                   lambda route: stream.StreamDecoder._prepare_band(decoder, A, route)),
    }


# (a covered band takes the streaming decoder on to torbi_hip_stream_band_prepare on the device: tests/test_stream_band_gpu.py)
@pytest.mark.parametrize('feature,matrix', [(f, m) for f in ('posteriors', 'sampling', 'k-best', 'stream') for m in MATRIX
                                            if f != 'stream' or m in ('none', 'uncovered')])
def test_features_raise_the_planner_s_reason_under_band_and_not_under_auto(monkeypatch, feature, matrix):
    """'band' on a matrix without a covered band: RuntimeError(who: why) from every feature, with `why` the planner's two
    texts and the feature's part in them; 'auto' goes dense there without raising, after the one look."""
    fakes = Fakes(monkeypatch, matrix)
    who, asked, call = features(monkeypatch, fakes)[feature]
    if matrix in ('none', 'uncovered'):
        finite = 'a finite value below every entry of the band' if feature == 'stream' else 'finite'
        why = NO_BAND.format(finite) if matrix == 'none' else f'{asked}, reach 1/2, background -20.0'
        with pytest.raises(RuntimeError) as raised:
            call('band')
        assert str(raised.value) == f'{who}: {why}' and fakes.looks == 1
        fakes.looks = 0
        assert call('auto') is None and fakes.looks == 1
    else:
        assert call('band') == BAND and fakes.looks == 1
        # (posteriors take every covered band; 4 diagonals of 64 states are a share of the row k-best's table holds at k = 2
        # -- 175 / 1440 -- and sampling's does not -- 23 / 1440)
        assert call('auto') == (None if feature == 'sampling' else BAND) and fakes.looks == 2


@pytest.mark.parametrize('matrix', MATRIX)
def test_counts_need_minus_inf_outside_the_band(monkeypatch, matrix):
    fakes = Fakes(monkeypatch, matrix)
    monkeypatch.setattr(training, '_counts_covered', fakes.covers)
    A = torch.zeros((S, S))
    with pytest.raises(RuntimeError, match="^route='band': ") as raised:           # BAND has a finite background
        training._counts_band(A, A, B, T, S, 0, 'band')
    assert fakes.asked == [] and fakes.looks == 1
    if matrix == 'none':
        assert str(raised.value) == "route='band': " + NO_BAND.format('finite')
    assert training._counts_band(A, A, B, T, S, 0, 'auto') is None and training._counts_band(A, A, B, T, S, 0, 'dense') is None
    assert fakes.looks == 2
    monkeypatch.setattr(viterbi, 'band_over', lambda *args: None if matrix == 'none' else (1, 2, -float('inf')))
    if matrix in ('covered', 'pays'):
        for route in ('band', 'auto'):
            assert training._counts_band(A, A, B, T, S, 0, route) == (1, 2)
    else:
        with pytest.raises(RuntimeError, match="^route='band': "):
            training._counts_band(A, A, B, T, S, 0, 'band')


def test_decode_k_best_auto_never_looks(monkeypatch):
    """`_routed(look=False)`, what `decode_k_best` passes: 'auto' on a matrix nobody has looked at asks nothing and goes
    dense; 'band' looks; 'auto' on a known structure takes what is known."""
    fakes = Fakes(monkeypatch, 'pays')
    monkeypatch.setattr(k_best, '_covered', fakes.covers)
    monkeypatch.setattr(k_best, '_run', lambda *args: 'dense')
    monkeypatch.setattr(k_best, '_run_band', lambda obs, frames, trans, init, k, *rest: rest[:3])
    x, f, pi = torch.zeros((B, T, 1440)), torch.full((B,), T), torch.zeros(1440)
    A = torch.zeros((1440, 1440))
    assert k_best._routed(x, f, A, A, None, pi, 2, 'auto', look=False) == 'dense' and fakes.looks == 0 and fakes.asked == []
    assert k_best._routed(x, f, A, A, None, pi, 2, 'band', look=False) == BAND and fakes.looks == 1
    state.notes(A)[('band_over', 1440)] = BAND
    assert k_best._routed(x, f, A, A, None, pi, 2, 'auto', look=False) == BAND and fakes.looks == 2
    # the caller's workspace must also hold the band layout, else 'auto' stays dense; 'band' leaves that to the call
    small = torch.empty(16, dtype=torch.uint8)
    assert k_best._routed(x, f, A, A, None, pi, 2, 'auto', small, look=False) == 'dense'
    assert k_best._routed(x, f, A, A, None, pi, 2, 'band', small, look=False) == BAND


def test_share_rule():
    """A band's width counts as its share of a row of 1440 states: the cases tests/test_sample_band_cpu.py and the k-best
    tests state, on the one rule both tables go through."""
    within = band_route.share_within
    assert within(1440, 11, 11, 23) and not within(1440, 12, 11, 23) and within(1440, 0, 0, 23)
    assert within(360, 2, 2, 23) and not within(360, 11, 11, 23) and not within(360, 3, 2, 23)         # 5.75 diagonals of 360
    assert within(1440, 87, 87, 175) and not within(1440, 88, 87, 175) and within(2880, 175, 174, 175)
    pays = sampling._band_pays
    assert pays(1, 1440, 11, 11, 1) and pays(512, 1440, 11, 11, 16) and pays(100, 360, 2, 2, 1)
    assert not pays(513, 1440, 11, 11, 1) and not pays(512, 1440, 12, 11, 1) and not pays(6, 360, 11, 11, 1)
    assert not pays(8, 1440, 11, 11, 2) and not pays(512, 1440, 11, 11, 17)
    pays = k_best._band_pays
    assert pays(4, 1440, 87, 87) and not pays(5, 1440, 87, 87) and not pays(12, 1440, 87, 87)            # (test_pitch_band)
    assert pays(8, 1440, 11, 11) and not pays(9, 1440, 11, 11) and not pays(8, 1440, 12, 11)
    assert pays(4, 64, 2, 2) and pays(3, 64, 3, 2) and pays(2, 64, 1, 1) and not pays(8, 64, 1, 1)       # 64 states: 7.7 and 1.02
