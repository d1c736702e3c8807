"""Which declared band route `band_route.route` asks, on the real torbi_hip_*_covers functions (host-only: they need no
device).  Only the look at the matrix is substituted -- `viterbi.band_over` reads a device tensor --, and it answers the band
of the case.  The three splits differ, and each is pinned here:

* state posteriors and path sampling: narrow iff min(W, S) <= 64, W the width after clamping each reach to S - 1.  On every
  case that is the first route whose covers function accepts.
* path entropy: narrow iff W <= 64, so 64 states with a wider band go to the wide route.
* expected counts: split like the posteriors, but a band inside the narrow window whose plane does not fit is the narrow
  route's to refuse, although the wide one would take it; and no route is asked about a finite background.
"""
import math

import pytest
import torch

from torbi_amd import _lib, band_route, entropy, posterior, sampling, training, viterbi

NINF = -math.inf
A = torch.zeros(1)                                                       # never read: the look is substituted
SHAPES = ((1, 1), (8, 500), (4096, 500))                                 # (B, T)
# (S, reaches): W <= 64 and W > 64 at 64 states; 68 states around the window; the pitch matrix's size with a plane that fits
# (0/22) and one that does not (0/26), around the window, wide, W = 511 > 512 - 3 and W = 513, which no route takes
BANDS = [(64, reach) for reach in ((1, 2), (1, 63), (31, 32), (32, 32), (63, 63), (200, 200))]
BANDS += [(68, reach) for reach in ((1, 2), (31, 32), (32, 32), (0, 66), (67, 67), (1, 67))]
BANDS += [(1440, reach) for reach in ((0, 22), (0, 26), (31, 32), (32, 32), (40, 30), (87, 87), (254, 254), (255, 255),
                                      (256, 256))]


def picked(monkeypatch, routes, shape, band, route='band'):
    """The index of the route `band_route.route` takes for `band`, None where it raises or goes dense."""
    monkeypatch.setattr(viterbi, 'band_over', lambda trans, original, states: band)
    try:
        taken = band_route.route(routes, route, A, A, shape, 0, 'who')
    except RuntimeError:
        return None
    return None if taken is None else routes.index(taken[0])


def first_that_covers(routes, shape, band):
    return next((k for k, r in enumerate(routes) if r.covers(*shape.values(), *band, 0)), None)


@pytest.mark.parametrize('background', [NINF, -20.])
def test_posteriors_and_sampling_take_the_first_route_that_covers(monkeypatch, background):
    seen = set()
    for (S, reach), (B, T) in ((band, shape) for band in BANDS for shape in SHAPES):
        band = (*reach, background)
        shapes = [(posterior._band_routes(), dict(batch=B, frames=T, states=S))]
        shapes += [(sampling._band_routes(), dict(batch=B, frames=T, states=S, draws=draws)) for draws in (1, 16)]
        for routes, shape in shapes:
            want = first_that_covers(routes, shape, band)
            assert picked(monkeypatch, routes, shape, band) == want, (shape, band)
            seen.add(want)
    assert seen == {0, 1, None}


def test_entropy_splits_on_the_uncapped_width(monkeypatch):
    shape = dict(batch=2, frames=3, states=64)
    for background in (NINF, -20.):
        assert picked(monkeypatch, entropy._band_routes(), shape, (1, 63, background)) == 1
        assert picked(monkeypatch, entropy._band_routes(), shape, (1, 2, background)) == 0
        # the same band of 65 > min(65, 64) entries is the narrow route's for the posteriors
        assert picked(monkeypatch, posterior._band_routes(), shape, (1, 63, background)) == 0
    for S, reach in BANDS:
        narrow = min(reach[0], S - 1) + min(reach[1], S - 1) + 1 <= 64
        for B, T in SHAPES:
            got = picked(monkeypatch, entropy._band_routes(), dict(batch=B, frames=T, states=S), (*reach, NINF))
            assert got in ((0, None) if narrow else (1, None)), (S, reach)


def test_counts_leave_a_narrow_band_whose_plane_does_not_fit_to_the_narrow_route(monkeypatch):
    routes = training._counts_routes()
    for B, T in SHAPES:
        shape = dict(batch=B, frames=T, states=1440)
        assert picked(monkeypatch, routes, shape, (0, 22, NINF)) == 0
        assert picked(monkeypatch, routes, shape, (40, 30, NINF)) == 1
        assert not posterior._counts_covered(B, T, 1440, 0, 26, NINF) and posterior._wide_counts_covered(B, T, 1440, 0, 26, NINF)
        monkeypatch.setattr(viterbi, 'band_over', lambda trans, original, states: (0, 26, NINF))
        with pytest.raises(RuntimeError, match=r"^route='band': .*torbi_hip_forward_backward_counts_band_covers.* turns down "
                                               rf'batch={B}, frames={T}, states=1440, reach 0/26, background -inf$'):
            training._counts_band(A, A, B, T, 1440, 0, 'band')
        assert training._counts_band(A, A, B, T, 1440, 0, 'auto') is None


class Spy:
    """The library, with the names that are looked up in it."""

    def __init__(self, lib):
        self.lib, self.asked = lib, []

    def __getattr__(self, name):
        self.asked.append(name)
        return getattr(self.lib, name)


def test_a_finite_background_never_reaches_a_counts_covers(monkeypatch):
    spy = Spy(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: spy)
    entries = ['torbi_hip_forward_backward_counts_band_covers', 'torbi_hip_forward_backward_counts_wide_band_covers']
    for S, reach in BANDS:
        shape = dict(batch=8, frames=500, states=S)
        for route in ('band', 'auto'):
            assert picked(monkeypatch, training._counts_routes(), shape, (*reach, -20.), route) is None
        assert spy.asked == []
        picked(monkeypatch, training._counts_routes(), shape, (*reach, NINF))
        assert spy.asked == [entries[min(min(reach[0], S - 1) + min(reach[1], S - 1) + 1, S) > 64]], (S, reach)
        del spy.asked[:]
