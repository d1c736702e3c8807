"""How a call with a `route=` argument is sent to a band route or the dense one: ONE planner for every feature that has one.

    band, why = plan(trans, original, covers, entry, shape, index)      # is there a band, does the feature's route cover it
    band = choose(route, band, why, pays, who)                           # what `route` does with the answer
    taken = route(routes, route, trans, original, shape, index, who)     # both, over the band routes a feature declares

A feature declares its band routes as data, one `BandRoute` each in the order they are asked (state posteriors, expected
counts, path entropy and path sampling a narrow and a wide one, max-marginals one), and `route` answers (the route, the band)
or None for the dense route.  k-best decoding and the two streaming classes have one band route and extras of their own
(a plan without a look, a workspace check, a stated band) and call `plan` and `choose` themselves.
"""
import collections

import torch

from . import state, viterbi

ROUTES = ('auto', 'dense', 'band')
# the states of the matrix every table of measured classes was timed on (the reference's pitch matrix); a band's width counts
# as its share of a row
_MEASURED_STATES = 1440
NARROW_ENTRIES = 64                               # in-band entries of a matrix row the narrow band routes take

# One band route of a feature: `covers(*shape, reach_left, reach_right, background, index)` over its torbi_hip_*_covers, `entry`
# that function's name for a refusal, `run` the call of its kernel, `classes` the table of (smallest batch, largest batch,
# diagonals of 1440 states[, most draws]) 'auto' takes it in (None: every covered band pays), and `takes(states, reach_left,
# reach_right)`: this route is the one to ask for this band.
BandRoute = collections.namedtuple('BandRoute', 'covers entry run classes takes')


def check_route(route, error=RuntimeError) -> str:
    if route not in ROUTES:
        raise error(f"route must be 'auto', 'dense' or 'band'; got {route!r}")
    return route


def stated(reach_left, reach_right, background):
    """The band a caller states, as (int, int, float)."""
    reach_left, reach_right, background = int(reach_left), int(reach_right), float(background)
    if reach_left < 0 or reach_right < 0:
        raise RuntimeError(f'reach_left and reach_right must be >= 0; got {reach_left}, {reach_right}')
    return reach_left, reach_right, background


def share_within(states: int, reach_left: int, reach_right: int, diagonals: int) -> bool:
    """The band holds at most `diagonals` / 1440 of a matrix row."""
    return (reach_left + reach_right + 1) * _MEASURED_STATES <= diagonals * states


def entries(states: int, reach_left: int, reach_right: int, cap: bool = True) -> int:
    """The in-band entries of a matrix row: the width of the band after clamping each reach to states - 1, and with `cap` at
    most the row itself."""
    width = min(reach_left, states - 1) + min(reach_right, states - 1) + 1
    return min(width, states) if cap else width


def narrow(states: int, reach_left: int, reach_right: int) -> bool:
    """`BandRoute.takes` of a narrow route: at most 64 in-band entries in a row."""
    return entries(states, reach_left, reach_right) <= NARROW_ENTRIES


def any_width(states: int, reach_left: int, reach_right: int) -> bool:
    """`BandRoute.takes` of a feature's last route: whatever the routes before it left."""
    return True


def taking(routes, states: int, reach_left: int, reach_right: int):
    """The first of the declared `routes` whose `takes` holds for this band: the one to ask, and the one that runs it."""
    return next(r for r in routes if r.takes(states, reach_left, reach_right))


def in_classes(table, batch: int, states: int, reach_left: int, reach_right: int, draws=None) -> bool:
    """The call lies in a class of `table`, entries (smallest batch, largest batch, diagonals of 1440 states[, most draws])."""
    return any(low <= batch <= high and share_within(states, reach_left, reach_right, diagonals)
               and (not most or draws <= most[0]) for low, high, diagonals, *most in table)


def plan(trans: torch.Tensor, original: torch.Tensor, covers, entry: str, shape: dict, index: int = 0, look: bool = True,
         finite: str = 'finite'):
    """((reach_left, reach_right, background), '') where a band route takes the prepared device matrix `trans` (`original`:
    the caller's tensor, which the look is remembered with), else (None, the reason).  The structure is what
    `viterbi.band_over` answers -- one look per tensor version; an unseen matrix while a stream is capturing has no band --,
    the shape what the feature's `covers(*shape.values(), reach_left, reach_right, background, index)` takes.  `shape` is the
    call in the order of that function, batch=, states= and what else it asks about; `entry` names the function (or is a
    callable that names it for the band found, where `covers` asks one of two routes) and `finite` says what a finite
    background has to be, both for the reason.  Without `look` only a structure that is already known
    counts: the look is a small kernel, a host synchronisation and, the first time, a device allocation."""
    states = shape['states']
    if shape['batch'] < 1:
        return None, 'the batch is empty'
    if not look:
        known = state.peek(original)
        if known is None or ('band_over', states) not in known:
            return None, 'the structure of the matrix is not known yet'
    over = viterbi.band_over(trans, original, states)
    if over is None:
        return None, ('the matrix does not hold one value outside a band that viterbi.band_over can answer for '
                      f'(states % 4 == 0, 64 <= states <= {viterbi.BAND_MAX_STATES}, reach_left + reach_right + 4 <= '
                      f'{viterbi.BAND_MAX_WINDOW}, a background that is -inf or {finite})')
    if not covers(*shape.values(), *over, index):
        asked = ', '.join(f'{name}={value}' for name, value in shape.items())
        name = entry(*over) if callable(entry) else entry
        return None, f'{name} turns down {asked}, reach {over[0]}/{over[1]}, background {over[2]}'
    return over, ''


def choose(route: str, band, why: str, pays, who: str):
    """The band `route` takes, or None for the dense route: 'dense' never takes one, 'band' takes `band` or raises
    RuntimeError(`who`: `why`), 'auto' takes it where `pays(reach_left, reach_right, background)` says so (None: the band
    route won in every class that was measured).  A caller that must not look at the matrix under 'dense' does not ask
    for a plan there."""
    if route == 'dense':
        return None
    if route == 'band':
        if band is None:
            raise RuntimeError(f'{who}: {why}')
        return band
    return band if band is not None and (pays is None or pays(*band)) else None


def route(routes, route: str, trans: torch.Tensor, original: torch.Tensor, shape: dict, index: int, who: str, look: bool = True):
    """(the BandRoute, (reach_left, reach_right, background)) where `route` sends the device matrix to one of the band routes
    a feature declares, else None for the dense route.  'dense' asks nothing; else one `plan`, so one look at the matrix, in
    which the first of `routes` whose `takes` holds for the band found is the only one whose `covers` is asked, and the one a
    refusal names; then `choose`, with that route's `classes` (read with batch=, states= and draws= of `shape`) for 'auto'."""
    if route == 'dense':
        return None
    states = shape['states']
    band, why = plan(trans, original, lambda *call: taking(routes, states, *call[-4:-2]).covers(*call),
                     lambda left, right, background: taking(routes, states, left, right).entry, shape, index, look)
    asked = None if band is None else taking(routes, states, *band[:2])
    pays = None if asked is None or asked.classes is None else lambda left, right, background: in_classes(
        asked.classes, shape['batch'], states, left, right, shape.get('draws'))
    band = choose(route, band, why, pays, who)
    return None if band is None else (asked, band)
